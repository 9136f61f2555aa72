"""Query by example over window embeddings: an index of embeddings resident on the device, and the exact top-k of a query against it.

:func:`avex_amd.recordings.embed_recordings` leaves one embedding per sliding window on the device, with each window's recording and
time span.  :class:`EmbeddingIndex` keeps such rows -- from any source -- as a list of chunks of ``chunk_rows`` prepared rows and answers
"here is one call, where are the others": scores, rows and the hits' recording / start / end, for ``k`` up to 1 024 and any number of rows
that fits in device memory.  The arithmetic runs in ``libavexhip.so`` (``csrc/search.hip``); there is no CPU fallback.

Semantics (the tests hold them; ``tests/_search_ref.py`` restates them in NumPy):

* **Rows.**  ``metric="cosine"``: a row is divided by ``max(||row||, 1e-12)`` in fp32 when it is added, a query when it is searched;
  ``metric="dot"``: rows and queries are taken as they are.  Inputs of any float dtype are converted to fp32 on the device.  The
  similarity is the fp32 dot product of the two prepared rows; it depends on those two rows only -- not on ``chunk_rows``, on
  ``batch_size``, or on the pieces the rows were added in.
* **Order.**  Higher similarity first, then lower row.  A NaN similarity is never a hit.  ``-0.0`` is returned as ``0.0``.
* **k.**  ``1 <= k <= 1024``.  ``count[q]`` hits are valid; past them ``rows`` / ``recording`` are ``-1``, ``scores`` ``-inf``, ``start_s`` /
  ``end_s`` NaN.  A ``k`` larger than the index is fine.
* **exclude** (needs ``query_recording``; ``"overlap"`` needs ``query_start_s`` / ``query_end_s`` too; otherwise ``ValueError``):
  ``"recording"`` drops the rows of the query's recording, ``"overlap"`` those of them whose span overlaps the query's by a positive
  amount, ``min(end) > max(start)``.  A query whose recording is ``-1`` excludes nothing.  Exclusion happens before selection: it never
  eats into ``k``.
* **nms=max_overlap** (a float in ``[0, 1)``): the ``K' = min(k * overfetch, 1024)`` best candidates are taken best first; a candidate is
  dropped if a hit already kept has the same ``recording >= 0`` and ``min(end) - max(start) > max_overlap * min(len_a, len_b)`` (fp64, as
  NumPy computes it).  With ``max_overlap=0.0`` windows that only touch survive.  Selection stops at ``k`` kept hits; there may be fewer.
  Rows without metadata (``recording = -1``) are never suppressed and never suppress.  Without ``nms``, ``K' = k``.
* A NaN span (a row added with a recording but no ``start_s`` / ``end_s``) behaves as in NumPy: ``min`` / ``max`` carry the NaN and every
  compare with it is false, so such a row is not excluded by ``"overlap"``, excludes nothing as a query, and neither suppresses nor is
  suppressed.
* ``search_rows`` takes its queries from the index: the prepared rows themselves (not normalised a second time) with their metadata, the
  query's own row never returned, ``exclude="overlap"`` unless told otherwise.

Nothing here synchronises with the host; results are device tensors.  Working memory is ``O(batch_size x chunk_rows + batch_size x K')``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._metric_inputs import _as_tensor, _stream

MAX_K = 1024                   # avexhip_search_max_k(): the depth of a running list
MAX_ROWS = (1 << 31) - 1       # rows of one index: a row is 32 key bits
METRICS = ("cosine", "dot")
EXCLUDES = (None, "recording", "overlap")
_DPAD = 32                     # a prepared row is padded to the K tile of the fp32 product

__all__ = ["EmbeddingIndex", "query_by_example", "MAX_K"]


def _dpad_of(d: int) -> int:
    return (int(d) + _DPAD - 1) // _DPAD * _DPAD


def _shape2(x) -> tuple:
    return tuple(x.shape) if isinstance(x, torch.Tensor) else np.asarray(x).shape


def _check_search_args(k, nms, overfetch, exclude, batch_size) -> int:
    """The list depth K' of a search, after the argument checks that need no GPU."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k={k!r}: an integer in 1..{MAX_K} expected")
    if isinstance(overfetch, bool) or not isinstance(overfetch, (int, np.integer)) or int(overfetch) < 1:
        raise ValueError(f"overfetch={overfetch!r}: an integer >= 1 expected")
    if nms is not None and (isinstance(nms, bool) or not isinstance(nms, (int, float, np.floating, np.integer)) or not 0.0 <= float(nms) < 1.0):
        raise ValueError(f"nms={nms!r}: None or a float in [0, 1) expected")
    if exclude not in EXCLUDES:
        raise ValueError(f"exclude={exclude!r}: one of {EXCLUDES} expected")
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or int(batch_size) < 1:
        raise ValueError(f"batch_size={batch_size!r}: a positive integer expected")
    return int(k) if nms is None else min(int(k) * int(overfetch), MAX_K)


class EmbeddingIndex:
    """Embeddings resident on the device with, per row, a recording id (int32, ``-1`` = none) and a time span in seconds (float64).

    ``add`` / ``add_recording`` / ``from_recordings`` fill it; ``search`` / ``search_rows`` query it; ``state_dict`` / ``from_state_dict``
    move it through host arrays.  See the module docstring for what a search returns.
    """

    def __init__(self, dim: int, metric: str = "cosine", device: Any = None, chunk_rows: int = 65536) -> None:
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or int(dim) < 1:
            raise ValueError(f"dim={dim!r}: a positive integer expected")
        if metric not in METRICS:
            raise ValueError(f"metric={metric!r}: one of {METRICS} expected")
        if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, (int, np.integer)) or not 1 <= int(chunk_rows) <= MAX_ROWS:
            raise ValueError(f"chunk_rows={chunk_rows!r}: an integer in 1..{MAX_ROWS} expected")
        self.dim, self.metric, self.chunk_rows = int(dim), metric, int(chunk_rows)
        self.dpad = _dpad_of(self.dim)
        self._device_arg = device
        self._device: Optional[torch.device] = None
        self._chunks: List[torch.Tensor] = []         # [capacity, dpad] fp32 each; every chunk but the last holds chunk_rows rows
        self._n = 0
        self._rec: Optional[torch.Tensor] = None      # [capacity] int32 / float64 / float64: the metadata of every row, in one piece
        self._start: Optional[torch.Tensor] = None
        self._end: Optional[torch.Tensor] = None
        self.names: List[str] = []

    # ------------------------------------------------------------------------------------------------------------------ filling
    def __len__(self) -> int:
        return self._n

    @property
    def n_recordings(self) -> int:
        return len(self.names)

    @property
    def device(self) -> torch.device:
        """The device of the index (initialises the GPU on first use)."""
        if self._device is None:
            _capi.require_gpu()
            dev = torch.device(self._device_arg) if self._device_arg is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _capi.AvexHipError(f"an index lives on a GPU, not on {dev} (there is no CPU fallback)")
            self._device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        return self._device

    def _meta_column(self, x, n: int, what: str, dtype: torch.dtype) -> Optional[torch.Tensor]:
        """A per-row metadata argument (scalar, array, tensor or None) as a host or device tensor of ``n`` entries; None stays None."""
        if x is None:
            return None
        if isinstance(x, (int, float, np.integer, np.floating)):
            return torch.full((n,), x, dtype=dtype)
        t = _as_tensor(x)
        if t.dim() != 1 or int(t.shape[0]) != n:
            raise ValueError(f"{what} holds {tuple(t.shape)} entries for {n} rows")
        return t

    def _grow_meta(self, need: int) -> None:
        cap = 0 if self._rec is None else int(self._rec.shape[0])
        if need <= cap:
            return
        new = max(need, 2 * cap, 1024)
        dev = self.device
        rec = torch.full((new,), -1, dtype=torch.int32, device=dev)
        start = torch.full((new,), float("nan"), dtype=torch.float64, device=dev)
        end = torch.full((new,), float("nan"), dtype=torch.float64, device=dev)
        if self._n:
            rec[:self._n].copy_(self._rec[:self._n])
            start[:self._n].copy_(self._start[:self._n])
            end[:self._n].copy_(self._end[:self._n])
        self._rec, self._start, self._end = rec, start, end

    def _open_chunk(self, rows_wanted: int) -> torch.Tensor:
        """The last chunk with room for at least one more row.  A chunk that is not full yet may move to a larger buffer (at most
        chunk_rows rows); a filled chunk never moves."""
        fill = self._n - (len(self._chunks) - 1) * self.chunk_rows if self._chunks else 0
        if not self._chunks or fill == self.chunk_rows:
            cap = min(self.chunk_rows, max(rows_wanted, 256))
            self._chunks.append(torch.empty((cap, self.dpad), dtype=torch.float32, device=self.device))
            return self._chunks[-1]
        last = self._chunks[-1]
        cap = int(last.shape[0])
        if fill == cap:
            bigger = torch.empty((min(self.chunk_rows, max(2 * cap, fill + rows_wanted)), self.dpad), dtype=torch.float32, device=self.device)
            bigger[:fill].copy_(last[:fill])
            self._chunks[-1] = last = bigger
        return last

    def _append(self, x: torch.Tensor, normalise: bool) -> None:
        """Rows [n, dim] fp32 on the device -> prepared rows at the end of the chunk list."""
        lib, s = _capi.lib(), _stream()
        n, done = int(x.shape[0]), 0
        while done < n:
            chunk = self._open_chunk(n - done)
            fill = self._n - (len(self._chunks) - 1) * self.chunk_rows
            take = min(n - done, int(chunk.shape[0]) - fill)
            _capi.check(lib.avexhip_search_prepare_rows(x.data_ptr() + 4 * done * x.stride(0), x.stride(0), take, self.dim, int(normalise),
                                                        chunk.data_ptr() + 4 * fill * self.dpad, s), "search_prepare_rows")
            done += take
            self._n += take

    def add(self, embeddings, recording=None, start_s=None, end_s=None) -> range:
        """Append ``embeddings [n, dim]`` (NumPy or torch, host or device; a device tensor is never copied to the host).  ``recording``: one
        id for all rows or one per row (``None``: ``-1``, no metadata); ``start_s`` / ``end_s``: the rows' spans in seconds, both or
        neither.  Returns the rows' global numbers.  Adding in pieces gives the same index, bit for bit, as adding at once.

        Ids given on the host (a scalar, a list, an array, a CPU tensor) are registered: ``names`` grows to cover them, an id without a
        name being named by its number.  Ids given as a device tensor are stored but not read back (``add`` never synchronises), so
        ``names`` / ``n_recordings`` do not learn of them: register such recordings with ``add_recording`` or one scalar ``add`` each if
        ``names[id]`` is to work."""
        shape = _shape2(embeddings)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"embeddings of shape {shape}: [n, {self.dim}] expected")
        n = int(shape[0])
        if (start_s is None) != (end_s is None):
            raise ValueError("start_s and end_s come together")
        rec = self._meta_column(recording, n, "recording", torch.int32)
        start = self._meta_column(start_s, n, "start_s", torch.float64)
        end = self._meta_column(end_s, n, "end_s", torch.float64)
        if self._n + n > MAX_ROWS:
            raise ValueError(f"{self._n + n} rows: more than 2^31 - 1 in one index")
        first = self._n
        if n == 0:
            return range(first, first)
        if rec is not None and not rec.is_cuda:            # ids the host can see are registered; a device tensor is not read back
            top = int(rec.max())
            while len(self.names) <= top:
                self.names.append(str(len(self.names)))
        dev = self.device
        with torch.cuda.device(dev):
            x = _as_tensor(embeddings).to(dev).to(torch.float32)
            if x.stride(1) != 1:
                x = x.contiguous()
            self._grow_meta(first + n)
            for col, val in ((self._rec, rec), (self._start, start), (self._end, end)):
                if val is not None:
                    col[first:first + n].copy_(val.to(col.dtype), non_blocking=True)
            self._append(x, self.metric == "cosine")
        return range(first, first + n)

    def add_recording(self, result: Dict[str, Any], name: Optional[str] = None) -> int:
        """Append the windows of one recording: ``result`` is a dict from :func:`avex_amd.recordings.embed_recording` /
        ``embed_recordings`` whose aggregation gives ``[n, dim]`` embeddings.  Returns the recording's id; ``names[id]`` is ``name``."""
        emb = result["embeddings"]
        if isinstance(emb, (list, tuple)):
            raise ValueError("one embedding per window expected (one layer, an aggregation that gives [n, dim])")
        n = len(result["start_s"])
        if not (len(_shape2(emb)) == 2 and _shape2(emb) == (n, self.dim)) and not (n == 0 and int(np.prod(_shape2(emb))) == 0):
            raise ValueError(f"embeddings of shape {_shape2(emb)}: [{n}, {self.dim}] expected")
        rid = len(self.names)
        self.names.append(str(rid) if name is None else str(name))
        if n:
            self.add(emb, recording=rid, start_s=np.asarray(result["start_s"], dtype=np.float64), end_s=np.asarray(result["end_s"], dtype=np.float64))
        return rid

    @classmethod
    def from_recordings(cls, model: Any, sources: Sequence[Any], window_s: float, hop_s: Optional[float] = None, *, metric: str = "cosine",
                        chunk_rows: int = 65536, names: Optional[Sequence[str]] = None, **embed_keywords) -> "EmbeddingIndex":
        """Embed every window of ``sources`` (:func:`avex_amd.recordings.embed_recordings`, which takes ``embed_keywords``) and index them;
        recording ``r`` is ``sources[r]``, named by its path when it is one."""
        from . import recordings
        if metric not in METRICS:
            raise ValueError(f"metric={metric!r}: one of {METRICS} expected")
        if names is not None and len(names) != len(sources):
            raise ValueError(f"{len(names)} names for {len(sources)} recordings")
        results = recordings.embed_recordings(model, list(sources), window_s, hop_s, **embed_keywords)
        full = [r["embeddings"] for r in results if not isinstance(r["embeddings"], (list, tuple)) and r["embeddings"].dim() == 2]
        if not full:
            raise ValueError("no window was embedded to an [n, dim] tensor: nothing to index")
        index = cls(int(full[0].shape[1]), metric=metric, device=full[0].device, chunk_rows=chunk_rows)
        for r, (src, res) in enumerate(zip(sources, results)):
            name = names[r] if names is not None else (os.fspath(src) if isinstance(src, (str, os.PathLike)) else None)
            index.add_recording(res, name=name)
        return index

    # ------------------------------------------------------------------------------------------------------------------ state
    def state_dict(self) -> Dict[str, np.ndarray]:
        """Host arrays, ``np.savez``-able: the prepared rows ``[n, dim]``, the metadata, the names, the metric and the chunk size."""
        n = self._n
        if n:
            rows = torch.cat([c[:min(self.chunk_rows, n - i * self.chunk_rows), :self.dim] for i, c in enumerate(self._chunks)]).cpu().numpy()
            rec, start, end = self._rec[:n].cpu().numpy(), self._start[:n].cpu().numpy(), self._end[:n].cpu().numpy()
        else:
            rows = np.zeros((0, self.dim), dtype=np.float32)
            rec, start, end = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.float64)
        return {"rows": rows, "recording": rec, "start_s": start, "end_s": end, "names": np.asarray(self.names, dtype=str),
                "metric": np.asarray(self.metric), "dim": np.asarray(self.dim, dtype=np.int64), "chunk_rows": np.asarray(self.chunk_rows, dtype=np.int64)}

    @classmethod
    def from_state_dict(cls, state: Dict[str, Any], device: Any = None) -> "EmbeddingIndex":
        """The index a ``state_dict`` was taken from: the prepared rows are copied back as they are, so searches give the same bits."""
        rows = np.asarray(state["rows"], dtype=np.float32)
        index = cls(int(state["dim"]), metric=str(state["metric"]), device=device, chunk_rows=int(state["chunk_rows"]))
        if rows.ndim != 2 or rows.shape[1] != index.dim:
            raise ValueError(f"rows of shape {rows.shape}: [n, {index.dim}] expected")
        n = rows.shape[0]
        for key in ("recording", "start_s", "end_s"):
            if np.asarray(state[key]).shape != (n,):
                raise ValueError(f"{key} holds {np.asarray(state[key]).shape} entries for {n} rows")
        index.names = [str(s) for s in np.asarray(state["names"]).reshape(-1).tolist()]
        if n:
            dev = index.device
            with torch.cuda.device(dev):
                index._grow_meta(n)
                index._rec[:n].copy_(torch.from_numpy(np.ascontiguousarray(state["recording"], dtype=np.int32)))
                index._start[:n].copy_(torch.from_numpy(np.ascontiguousarray(state["start_s"], dtype=np.float64)))
                index._end[:n].copy_(torch.from_numpy(np.ascontiguousarray(state["end_s"], dtype=np.float64)))
                index._append(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), False)
        return index

    # ------------------------------------------------------------------------------------------------------------------ searching
    def _query_meta(self, nq: int, exclude, query_recording, query_start_s, query_end_s):
        """Host-side checks of the query's metadata -> host / device tensors (or None)."""
        if exclude is not None and query_recording is None:
            raise ValueError(f"exclude={exclude!r} needs query_recording")
        if exclude == "overlap" and (query_start_s is None or query_end_s is None):
            raise ValueError("exclude='overlap' needs query_start_s and query_end_s")
        if isinstance(query_recording, str):
            if query_recording not in self.names:
                raise ValueError(f"no recording named {query_recording!r}")
            query_recording = self.names.index(query_recording)
        return (self._meta_column(query_recording, nq, "query_recording", torch.int32),
                self._meta_column(query_start_s, nq, "query_start_s", torch.float64),
                self._meta_column(query_end_s, nq, "query_end_s", torch.float64))

    def search(self, query, k: int = 10, *, nms: Optional[float] = None, overfetch: int = 4, exclude: Optional[str] = None, query_recording=None,
               query_start_s=None, query_end_s=None, batch_size: int = 1024, return_sim: bool = False, _timing: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """The ``k`` best rows for every row of ``query [nq, dim]``: device tensors ``scores [nq, k]`` fp32, ``rows [nq, k]`` int64,
        ``count [nq]`` int32, ``recording [nq, k]`` int32, ``start_s`` / ``end_s [nq, k]`` fp64, and with ``return_sim`` (tests, small sets)
        ``sim [nq, len(index)]``.  ``query_recording``: an id (or a name) for all queries, or one id per query; the spans likewise.  See the
        module docstring for the semantics.  ``_timing`` (a dict, for ``scripts/search_bench.py``) launches the stages separately with
        events between them and receives ``similarity_s`` / ``select_s`` / ``finish_s``; the results are the same."""
        shape = _shape2(query)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"query of shape {shape}: [nq, {self.dim}] expected")
        kp = _check_search_args(k, nms, overfetch, exclude, batch_size)
        qmeta = self._query_meta(int(shape[0]), exclude, query_recording, query_start_s, query_end_s)
        if self._n == 0:
            raise ValueError("the index is empty")
        dev = self.device
        with torch.cuda.device(dev):
            q = _as_tensor(query).to(dev).to(torch.float32).contiguous()
            return self._search(q, self.metric == "cosine", int(k), kp, nms, exclude, qmeta, None, int(batch_size), return_sim, _timing)

    def search_rows(self, rows, k: int = 10, *, nms: Optional[float] = None, overfetch: int = 4, exclude: Optional[str] = "overlap", batch_size: int = 1024,
                    return_sim: bool = False) -> Dict[str, torch.Tensor]:
        """:meth:`search` with indexed rows as the queries: their prepared embeddings and their metadata are taken from the index on the
        device, a query's own row is never returned, and ``exclude`` defaults to ``"overlap"`` (a row without metadata excludes nothing).
        ``rows``: a list / array of global row numbers (checked here) or a device tensor (not copied back: a number outside the index is
        clamped into it)."""
        kp = _check_search_args(k, nms, overfetch, exclude, batch_size)
        if self._n == 0:
            raise ValueError("the index is empty")
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            r = rows.reshape(-1)
        else:
            a = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows)
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError("rows: a 1-d integer list expected")
            if a.size and (int(a.min()) < 0 or int(a.max()) >= self._n):
                raise ValueError(f"rows outside 0..{self._n - 1}")
            r = torch.from_numpy(a.astype(np.int64))
        dev = self.device
        with torch.cuda.device(dev):
            r = r.to(dev).to(torch.int64).clamp(0, self._n - 1).contiguous()
            nq = int(r.shape[0])
            q = torch.zeros((nq, self.dpad), dtype=torch.float32, device=dev)
            for i, c in enumerate(self._chunks):           # a gather per chunk, blended by a mask: no copy to the host, no synchronisation
                r0 = i * self.chunk_rows
                nc = min(self.chunk_rows, self._n - r0)
                inside = (r >= r0) & (r < r0 + nc)
                q = torch.where(inside[:, None], c[(r - r0).clamp(0, nc - 1)], q)
            qmeta = (self._rec[r].contiguous(), self._start[r].contiguous(), self._end[r].contiguous()) if exclude is not None else (None, None, None)
            return self._search(q[:, :self.dim], False, int(k), kp, nms, exclude, qmeta, r, int(batch_size), return_sim, None)

    def _search(self, q: torch.Tensor, normalise: bool, k: int, kp: int, nms, exclude, qmeta, skip: Optional[torch.Tensor], batch_size: int,
                return_sim: bool, timing: Optional[dict]) -> Dict[str, torch.Tensor]:
        dev, lib, s = self.device, _capi.lib(), _stream()
        nq, n = int(q.shape[0]), self._n
        qrec, qstart, qend = (None if t is None else t.to(dev).contiguous() for t in qmeta)
        out = {"scores": torch.empty((nq, k), dtype=torch.float32, device=dev), "rows": torch.empty((nq, k), dtype=torch.int64, device=dev),
               "count": torch.empty((nq,), dtype=torch.int32, device=dev), "recording": torch.empty((nq, k), dtype=torch.int32, device=dev),
               "start_s": torch.empty((nq, k), dtype=torch.float64, device=dev), "end_s": torch.empty((nq, k), dtype=torch.float64, device=dev)}
        sim = torch.empty((nq, n), dtype=torch.float32, device=dev) if return_sim else None
        if return_sim:
            out["sim"] = sim
        if nq == 0:
            return out
        batch = min(batch_size, nq)
        walk = min(self.chunk_rows, n)                     # rows of the largest chunk: what the workspace is sized for
        ws_bytes = int(lib.avexhip_search_workspace_bytes(walk, self.dim, batch, kp))
        if ws_bytes == 0:
            raise _capi.AvexHipError(f"search: no workspace for chunk_rows {walk}, dim {self.dim}, batch {batch}, k {kp}")
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        a = _capi.SearchArgs()
        a.d, a.batch, a.k, a.chunk_rows, a.normalise = self.dim, batch, kp, walk, int(normalise)
        a.exclude = EXCLUDES.index(exclude)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        r = _capi.SearchResult()
        r.k, r.nms, r.max_overlap, r.n_rows = k, int(nms is not None), float(nms or 0.0), n
        r.db_recording, r.db_start, r.db_end = self._rec.data_ptr(), self._start.data_ptr(), self._end.data_ptr()
        marks = []
        for b0 in range(0, nq, batch):
            nb = min(batch, nq - b0)
            a.nb = nb
            a.query, a.ld_query = q.data_ptr() + 4 * b0 * q.stride(0), q.stride(0)
            a.skip_row = skip.data_ptr() + 8 * b0 if skip is not None else None
            a.query_recording = qrec.data_ptr() + 4 * b0 if exclude is not None else None
            a.query_start = qstart.data_ptr() + 8 * b0 if exclude == "overlap" else None
            a.query_end = qend.data_ptr() + 8 * b0 if exclude == "overlap" else None
            _capi.check(lib.avexhip_search_begin(C.byref(a), s), "search_begin")
            for i, c in enumerate(self._chunks):
                r0 = i * self.chunk_rows
                a.chunk, a.row0, a.n_rows = c.data_ptr(), r0, min(self.chunk_rows, n - r0)
                a.db_recording = self._rec.data_ptr() + 4 * r0 if exclude is not None else None
                a.db_start = self._start.data_ptr() + 8 * r0 if exclude == "overlap" else None
                a.db_end = self._end.data_ptr() + 8 * r0 if exclude == "overlap" else None
                a.sim_out, a.ld_sim = (sim.data_ptr() + 4 * (b0 * n + r0), n) if return_sim else (None, 0)
                if timing is None:
                    a.stages = 3
                    _capi.check(lib.avexhip_search_chunk(C.byref(a), s), "search_chunk")
                    continue
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                for stage in (1, 2):
                    a.stages = stage
                    _capi.check(lib.avexhip_search_chunk(C.byref(a), s), "search_chunk")
                    ev[stage].record()
                marks.append(ev)
            for name in ("scores", "rows", "recording", "start_s", "end_s"):
                setattr(r, name, out[name].data_ptr() + out[name].element_size() * b0 * k)
            r.count = out["count"].data_ptr() + 4 * b0
            if timing is not None:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
            _capi.check(lib.avexhip_search_finish(C.byref(a), C.byref(r), s), "search_finish")
            if timing is not None:
                ev[1].record()
                marks.append(ev)
        if timing is not None:
            torch.cuda.synchronize(dev)
            timing["similarity_s"] = sum(e[0].elapsed_time(e[1]) for e in marks if len(e) == 3) * 1e-3
            timing["select_s"] = sum(e[1].elapsed_time(e[2]) for e in marks if len(e) == 3) * 1e-3
            timing["finish_s"] = sum(e[0].elapsed_time(e[1]) for e in marks if len(e) == 2) * 1e-3
        return out


def query_by_example(model: Any, index: EmbeddingIndex, source: Any, k: int = 10, *, sr: int = 16000, target_len: Optional[int] = None,
                     aggregation: str = "mean", **search_keywords) -> Dict[str, torch.Tensor]:
    """Embed one clip -- ``source`` is a path or bytes (WAV / FLAC) or an array at ``sr`` -- through
    :func:`avex_amd.ingest.load_batch` and ``model.extract_embeddings`` with the layers the model has registered (its last layer when none
    is), then :meth:`EmbeddingIndex.search` with ``search_keywords``.  ``target_len`` pads or crops the clip (``None``: as it is)."""
    from . import ingest
    _check_search_args(k, search_keywords.get("nms"), search_keywords.get("overfetch", 4), search_keywords.get("exclude"), search_keywords.get("batch_size", 1024))
    if len(index) == 0:
        raise ValueError("the index is empty")
    wav, mask, _ = ingest.load_batch([source], sr, target_len, device=index.device)
    if not model._hook_layers:
        model.register_hooks_for_layers(["last_layer"])
    else:
        model.ensure_hooks_registered()
    with torch.no_grad():
        emb = model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation=aggregation)
    if isinstance(emb, (list, tuple)) or emb.dim() != 2:
        raise ValueError("one embedding per clip expected (one layer, an aggregation that gives [1, dim])")
    return index.search(emb, k, **search_keywords)
