"""Few-shot class scores from labelled example windows: a bank of example embeddings with a class each, and for every window to score
the mean of its ``top_m`` largest similarities to each class's examples.

A field recording is rarely annotated enough to train a head; what there usually is are a few marked calls per species and a pile of
"this is not it" clips.  :class:`ExampleBank` keeps their embeddings on the device, ``bank.score(emb)`` gives the ``[N, C]`` score matrix
:func:`avex_amd.detection.decode_events` reads, ``bank.scorer()`` is a ``probe`` for :func:`avex_amd.detection.detect_events`, and
:func:`detect_events_by_example` runs the whole chain from files.  No training.  The arithmetic runs in ``libavexhip.so``
(``csrc/examples.hip``); the ``[windows, examples]`` similarity matrix is never stored, and there is no CPU fallback.

Semantics (the tests hold them; ``tests/_examples_ref.py`` restates them in NumPy):

* **Bank.**  Every row has a label: a class ``0 .. C - 1`` or ``-1``, *background* (a negative example).  ``C`` is ``n_classes`` when
  given, else ``max(label) + 1``.  Rows are prepared as :class:`avex_amd.search.EmbeddingIndex` prepares them, by the same code:
  ``metric="cosine"`` divides by ``max(||row||, 1e-12)`` in fp32, ``metric="dot"`` copies; the windows to score likewise.
* **Similarity.**  The fp32 product of the search: for the same two rows, the bits ``EmbeddingIndex.search(..., return_sim=True)`` gives.
* **Per-class value** ``s[n, c]``, ``1 <= top_m <= 16``: of the similarities of window ``n`` to the rows of class ``c`` that are numbers (a
  NaN is never counted, ``-0.0`` is ``+0.0``), the ``min(top_m, count)`` largest, added in fp32 in descending order from the largest,
  divided by ``float(count kept)``.  None: NaN (an empty class, a NaN window).  ``s_bg[n]`` is the same over the background rows.
* **Modes.**  ``"similarity"``: ``scores = s``.  ``"margin"``: ``scores[n, c] = s[n, c] - s_bg[n]`` (NaN carries); needs background rows.
* **Nearest.**  ``nearest[n, c]`` (int32): the row, numbered in the order rows were added, with the highest similarity in class ``c``,
  the lower row on a tie; ``-1`` where no row gives a number.
* Scores do not depend on ``batch_size``, on the pieces or the order the rows were added in, or on the run: a score is a function of a
  multiset of similarities, and a similarity of its two rows.
* **Prototypes.**  ``bank.prototypes()`` is a bank of one row per non-empty class (and one background row if there are any): the fp32 sum
  of the class's prepared rows in the order they were added, from 0, over ``float(count)``, added through :meth:`ExampleBank.add` (so
  prepared again).  Scoring it with ``top_m=1`` is nearest-prototype scoring.

Nothing here synchronises with the host; results are device tensors.  Working memory is ``O(batch_size x segments x top_m)`` where a
segment is a class's share of a 128-row tile of the bank: at most ``ceil(M / 128) + C`` of them.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._metric_inputs import _as_tensor, _stream
from .search import METRICS, MAX_ROWS, _dpad_of, _shape2

MAX_TOP_M = 16                  # avexhip_examples_max_top_m(): the depth of a per-class list
MAX_CLASSES = 1 << 20           # classes of one bank
MAX_BATCH = 1 << 22             # windows of one launch: a larger batch_size is cut to it
MODES = ("similarity", "margin")
TILE = 128                      # bank rows per tile of the fp32 product

__all__ = ["ExampleBank", "detect_events_by_example", "segment_tables", "MAX_TOP_M"]


def _check_score_args(top_m, mode, batch_size) -> None:
    if isinstance(top_m, bool) or not isinstance(top_m, (int, np.integer)) or not 1 <= int(top_m) <= MAX_TOP_M:
        raise ValueError(f"top_m={top_m!r}: an integer in 1..{MAX_TOP_M} expected")
    if mode not in MODES:
        raise ValueError(f"mode={mode!r}: one of {MODES} expected")
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or int(batch_size) < 1:
        raise ValueError(f"batch_size={batch_size!r}: a positive integer expected")


def segment_tables(counts) -> Dict[str, np.ndarray]:
    """The host tables of a bank sorted by class.  ``counts [C + 1]``: rows per class, the background last.  A segment is a class's share
    of one tile of ``TILE`` sorted rows.  Returns int32 arrays: ``segments [S, 4]`` = (class, first column, last column, tile) in column
    order, ``tile_segments [T + 1]`` (the segments of tile ``t`` are ``tile_segments[t] .. tile_segments[t + 1] - 1``) and
    ``class_segments [C + 1, 2]`` = (first, last) segment of each class, ``(0, -1)`` for an empty one."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if counts.size < 1 or (counts < 0).any():
        raise ValueError("counts: one non-negative number per class, and one for the background, expected")
    ends = np.cumsum(counts)
    starts = ends - counts
    m = int(ends[-1])
    n_tiles = (m + TILE - 1) // TILE
    segs: List[np.ndarray] = []
    class_segments = np.empty((counts.size, 2), dtype=np.int32)
    n = 0
    for c in range(counts.size):
        if counts[c] == 0:
            class_segments[c] = (0, -1)
            continue
        tiles = np.arange(starts[c] // TILE, (ends[c] - 1) // TILE + 1, dtype=np.int64)
        first = np.maximum(tiles * TILE, starts[c])
        last = np.minimum(tiles * TILE + TILE - 1, ends[c] - 1)
        segs.append(np.stack([np.full_like(tiles, c), first, last, tiles], axis=1))
        class_segments[c] = (n, n + len(tiles) - 1)
        n += len(tiles)
    segments = (np.concatenate(segs) if segs else np.zeros((0, 4), dtype=np.int64)).astype(np.int32)
    tile_segments = np.searchsorted(segments[:, 3], np.arange(n_tiles + 1), side="left").astype(np.int32)
    return {"segments": np.ascontiguousarray(segments), "tile_segments": np.ascontiguousarray(tile_segments), "class_segments": class_segments}


class ExampleBank:
    """Example embeddings resident on the device with one label per row (a class, or ``-1`` for background).

    ``add`` / ``add_clips`` fill it; ``score`` / ``scorer`` score windows against it; ``prototypes`` condenses it to class means;
    ``state_dict`` / ``from_state_dict`` move it through host arrays.  See the module docstring for what a score is.
    """

    def __init__(self, dim: int, n_classes: Optional[int] = None, metric: str = "cosine", device: Any = None,
                 class_names: Optional[Sequence[str]] = None) -> None:
        if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or int(dim) < 1:
            raise ValueError(f"dim={dim!r}: a positive integer expected")
        if n_classes is not None and (isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or int(n_classes) < 1):
            raise ValueError(f"n_classes={n_classes!r}: None or a positive integer expected")
        if metric not in METRICS:
            raise ValueError(f"metric={metric!r}: one of {METRICS} expected")
        if class_names is not None and n_classes is not None and len(class_names) != int(n_classes):
            raise ValueError(f"{len(class_names)} class names for {n_classes} classes")
        self.dim, self.metric = int(dim), metric
        self._n_classes = None if n_classes is None else int(n_classes)
        self.class_names = None if class_names is None else [str(s) for s in class_names]
        self.dpad = _dpad_of(self.dim)
        self._device_arg = device
        self._device: Optional[torch.device] = None
        self._pieces: List[torch.Tensor] = []          # prepared rows [n_i, dpad] fp32 on the device, in the order they were added
        self._labels: List[np.ndarray] = []            # their labels, on the host
        self._n = 0
        self._max_label = -1
        self._layout: Optional[Dict[str, Any]] = None  # the class-sorted bank and its tables: made at the first score after the last add

    # ------------------------------------------------------------------------------------------------------------------ filling
    def __len__(self) -> int:
        return self._n

    @property
    def n_classes(self) -> int:
        """``C``: as given, else ``max(label) + 1`` of the rows added so far."""
        return self._n_classes if self._n_classes is not None else self._max_label + 1

    @property
    def labels(self) -> np.ndarray:
        """The label of every row, in the order they were added (int32, host)."""
        return np.concatenate(self._labels).astype(np.int32) if self._labels else np.zeros(0, dtype=np.int32)

    @property
    def counts(self) -> np.ndarray:
        """Rows per class ``[C + 1]`` (int64, host): classes ``0 .. C - 1``, then the background."""
        lab = self.labels.astype(np.int64)
        c = self.n_classes
        return np.bincount(np.where(lab < 0, c, lab), minlength=c + 1)

    @property
    def device(self) -> torch.device:
        """The device of the bank (initialises the GPU on first use)."""
        if self._device is None:
            _capi.require_gpu()
            dev = torch.device(self._device_arg) if self._device_arg is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _capi.AvexHipError(f"a bank lives on a GPU, not on {dev} (there is no CPU fallback)")
            self._device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        return self._device

    def _host_labels(self, labels, n: int) -> np.ndarray:
        if isinstance(labels, torch.Tensor):
            if labels.is_cuda:
                raise ValueError("labels live on the host (a list, an array or a CPU tensor): add never reads the device back")
            labels = labels.numpy()
        a = np.asarray(labels)
        if a.dtype.kind not in "iu" and a.size:
            raise ValueError(f"labels of dtype {a.dtype}: integers expected")
        if a.ndim == 0:
            a = np.full((n,), int(a))
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"labels holds {a.shape} entries for {n} rows")
        a = a.astype(np.int64)
        top = (self._n_classes if self._n_classes is not None else 1 << 31) - 1
        if a.size and (int(a.min()) < -1 or int(a.max()) > top):
            raise ValueError(f"labels outside -1..{top}" if self._n_classes is not None else "labels below -1 (background)")
        return a

    def _append(self, x: torch.Tensor, normalise: bool, lab: np.ndarray) -> range:
        """Rows [n, dim] fp32 on the device -> prepared rows at the end of the bank."""
        n, first = int(x.shape[0]), self._n
        out = torch.empty((n, self.dpad), dtype=torch.float32, device=self.device)
        _capi.check(_capi.lib().avexhip_search_prepare_rows(x.data_ptr(), x.stride(0), n, self.dim, int(normalise), out.data_ptr(), _stream()),
                    "search_prepare_rows")
        self._pieces.append(out)
        self._labels.append(lab)
        self._n += n
        self._max_label = max(self._max_label, int(lab.max()))
        self._layout = None
        return range(first, first + n)

    def add(self, embeddings, labels) -> range:
        """Append ``embeddings [n, dim]`` (NumPy or torch, any float dtype, host or device; a device tensor is never copied to the host)
        with ``labels``: one integer for all rows or one per row, on the host, a class ``0 .. C - 1`` or ``-1`` for background.  Returns
        the rows' numbers.  Adding in pieces, or in another order, gives the same scores bit for bit.  Never synchronises."""
        shape = _shape2(embeddings)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"embeddings of shape {shape}: [n, {self.dim}] expected")
        n = int(shape[0])
        lab = self._host_labels(labels, n)
        if self._n + n > MAX_ROWS:
            raise ValueError(f"{self._n + n} rows: more than 2^31 - 1 in one bank")
        if n == 0:
            return range(self._n, self._n)
        dev = self.device
        with torch.cuda.device(dev):
            x = _as_tensor(embeddings).to(dev).to(torch.float32)
            if x.stride(1) != 1:
                x = x.contiguous()
            return self._append(x, self.metric == "cosine", lab)

    def add_clips(self, model: Any, sources: Sequence[Any], labels, *, sr: int = 16000, target_len: Optional[int] = None,
                  aggregation: str = "mean") -> range:
        """Embed annotated clips the way :func:`avex_amd.search.query_by_example` embeds its query -- :func:`avex_amd.ingest.load_batch`,
        then ``model.extract_embeddings`` with the layers the model has registered (its last layer when none is) -- and add them.  A
        source is a path or bytes (WAV / FLAC) or an array at ``sr``, or ``(source, start_s, end_s)``: that span of it."""
        from . import ingest
        sources = list(sources)
        lab = self._host_labels(labels, len(sources))
        if not sources:
            return range(self._n, self._n)
        dev = self.device
        clips = []
        for src in sources:
            if isinstance(src, tuple):
                if len(src) != 3 or not float(src[1]) < float(src[2]) or float(src[1]) < 0.0:
                    raise ValueError("(source, start_s, end_s) with 0 <= start_s < end_s expected")
                wav, _, lengths = ingest.load_batch([src[0]], sr, None, device=dev)
                lo, hi = int(round(float(src[1]) * sr)), min(int(round(float(src[2]) * sr)), int(wav.shape[1]))
                if lo >= hi:
                    raise ValueError(f"the span {src[1]}..{src[2]} s lies outside the clip")
                clips.append(wav[0, lo:hi])
            else:
                clips.append(src)
        wav, mask, _ = ingest.load_batch(clips, sr, target_len, device=dev)
        if not model._hook_layers:
            model.register_hooks_for_layers(["last_layer"])
        else:
            model.ensure_hooks_registered()
        with torch.no_grad():
            emb = model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation=aggregation)
        if isinstance(emb, (list, tuple)) or emb.dim() != 2:
            raise ValueError("one embedding per clip expected (one layer, an aggregation that gives [n, dim])")
        return self.add(emb, lab)

    # ------------------------------------------------------------------------------------------------------------------ layout
    def _prepare(self) -> Dict[str, Any]:
        """The bank sorted by class (stable, background last) with its segment tables, on the device; made once after the last add."""
        if self._layout is not None:
            return self._layout
        dev, c = self.device, self.n_classes
        lab = self.labels.astype(np.int64)
        order = np.argsort(np.where(lab < 0, c, lab), kind="stable")
        counts = self.counts
        tables = segment_tables(counts)
        with torch.cuda.device(dev):
            rows = self._pieces[0] if len(self._pieces) == 1 else torch.cat(self._pieces)
            self._pieces = [rows]
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)      # noqa: E731
            order_dev = up(order)
            self._layout = {"bank": rows.index_select(0, order_dev).contiguous(), "row_id": up(order.astype(np.int32)), "counts": counts,
                            "n_segments": int(tables["segments"].shape[0]), **{k: up(v) for k, v in tables.items()}}
        return self._layout

    # ------------------------------------------------------------------------------------------------------------------ scoring
    def _check_ready(self, mode: str) -> None:
        if self._n == 0:
            raise ValueError("the bank is empty")
        if self.n_classes < 1:
            raise ValueError("the bank holds background rows only: no class to score")
        if self.n_classes > MAX_CLASSES:
            raise ValueError(f"{self.n_classes} classes: more than {MAX_CLASSES} in one bank")
        if mode == "margin" and not (self.labels < 0).any():
            raise ValueError("mode='margin' needs background rows (label -1)")

    def score(self, embeddings, *, top_m: int = 1, mode: str = "similarity", batch_size: int = 4096, return_nearest: bool = False,
              _timing: Optional[dict] = None):
        """``scores [N, C]`` fp32 on the device for ``embeddings [N, dim]``, or ``(scores, nearest [N, C] int32)`` with ``return_nearest``.
        See the module docstring for the semantics.  ``_timing`` (a dict, for ``scripts/examples_bench.py``) launches the two stages
        separately with events between them and receives ``tile_s`` / ``reduce_s``; the results are the same."""
        shape = _shape2(embeddings)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"embeddings of shape {shape}: [N, {self.dim}] expected")
        _check_score_args(top_m, mode, batch_size)
        self._check_ready(mode)
        dev, lib = self.device, _capi.lib()
        n, c = int(shape[0]), self.n_classes
        with torch.cuda.device(dev):
            q = _as_tensor(embeddings).to(dev).to(torch.float32)
            if n and q.stride(1) != 1:
                q = q.contiguous()
            scores = torch.empty((n, c), dtype=torch.float32, device=dev)
            nearest = torch.empty((n, c), dtype=torch.int32, device=dev) if return_nearest else None
            if n == 0:
                return (scores, nearest) if return_nearest else scores
            lay, s = self._prepare(), _stream()
            batch = min(int(batch_size), n, MAX_BATCH)
            ws_bytes = int(lib.avexhip_examples_workspace_bytes(batch, lay["n_segments"], int(top_m), self.dpad))
            if ws_bytes == 0:
                raise _capi.AvexHipError(f"examples: no workspace for batch {batch}, {lay['n_segments']} segments, top_m {top_m}, dpad {self.dpad}")
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            a = _capi.ExamplesArgs()
            a.bank, a.row_id, a.m, a.d, a.n_classes = lay["bank"].data_ptr(), lay["row_id"].data_ptr(), self._n, self.dim, c
            a.n_segments, a.batch = lay["n_segments"], batch
            a.segments, a.tile_segments, a.class_segments = lay["segments"].data_ptr(), lay["tile_segments"].data_ptr(), lay["class_segments"].data_ptr()
            a.top_m, a.mode, a.normalise = int(top_m), MODES.index(mode), int(self.metric == "cosine")
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
            a.ld_query, a.ld_scores, a.ld_nearest = q.stride(0), c, c
            marks = []
            for b0 in range(0, n, batch):
                a.n = min(batch, n - b0)
                a.query = q.data_ptr() + 4 * b0 * q.stride(0)
                a.scores = scores.data_ptr() + 4 * b0 * c
                a.nearest = nearest.data_ptr() + 4 * b0 * c if return_nearest else None
                if _timing is None:
                    a.stages = 3
                    _capi.check(lib.avexhip_examples_score(C.byref(a), s), "examples_score")
                    continue
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                for stage in (1, 2):
                    a.stages = stage
                    _capi.check(lib.avexhip_examples_score(C.byref(a), s), "examples_score")
                    ev[stage].record()
                marks.append(ev)
            if _timing is not None:
                torch.cuda.synchronize(dev)
                _timing["tile_s"] = sum(e[0].elapsed_time(e[1]) for e in marks) * 1e-3
                _timing["reduce_s"] = sum(e[1].elapsed_time(e[2]) for e in marks) * 1e-3
        return (scores, nearest) if return_nearest else scores

    def scorer(self, *, top_m: int = 1, mode: str = "similarity", batch_size: int = 4096) -> Callable[[torch.Tensor], torch.Tensor]:
        """A callable from ``[n, dim]`` embeddings to ``[n, C]`` scores: what :func:`avex_amd.detection.detect_events` takes as ``probe``."""
        _check_score_args(top_m, mode, batch_size)
        self._check_ready(mode)
        return lambda emb: self.score(emb, top_m=top_m, mode=mode, batch_size=batch_size)

    def prototypes(self) -> "ExampleBank":
        """A new bank of one row per non-empty class, and one background row if there are any: the class means (see the module docstring)."""
        c = self.n_classes                      # the prototype bank scores the same classes: empty ones stay empty
        names = self.class_names if self.class_names is not None and len(self.class_names) == c else None
        out = ExampleBank(self.dim, n_classes=c if c >= 1 else None, metric=self.metric, device=self._device_arg, class_names=names)
        if self._n == 0:
            return out
        dev, lib = self.device, _capi.lib()
        lay = self._prepare()
        counts = lay["counts"]
        keep = np.flatnonzero(counts)
        first = (np.cumsum(counts) - counts)[keep].astype(np.int32)
        labels = np.where(keep == self.n_classes, -1, keep)
        with torch.cuda.device(dev):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)      # noqa: E731
            first_dev, count_dev = up(first), up(counts[keep].astype(np.int32))
            means = torch.empty((len(keep), self.dim), dtype=torch.float32, device=dev)
            for k0 in range(0, len(keep), 65535):
                k1 = min(k0 + 65535, len(keep))
                _capi.check(lib.avexhip_examples_class_mean(lay["bank"].data_ptr(), self._n, self.dim, first_dev.data_ptr() + 4 * k0, count_dev.data_ptr() + 4 * k0,
                                                            k1 - k0, means.data_ptr() + 4 * k0 * self.dim, self.dim, _stream()), "examples_class_mean")
            out.add(means, labels)
        return out

    # ------------------------------------------------------------------------------------------------------------------ state
    def state_dict(self) -> Dict[str, np.ndarray]:
        """Host arrays, ``np.savez``-able: the prepared rows ``[n, dim]`` in the order they were added, their labels, the metric, the
        width, ``n_classes`` (``-1``: not given) and the class names."""
        rows = torch.cat(self._pieces)[:, :self.dim].cpu().numpy() if self._n else np.zeros((0, self.dim), dtype=np.float32)
        return {"rows": rows, "labels": self.labels, "metric": np.asarray(self.metric), "dim": np.asarray(self.dim, dtype=np.int64),
                "n_classes": np.asarray(-1 if self._n_classes is None else self._n_classes, dtype=np.int64),
                "class_names": np.asarray([] if self.class_names is None else self.class_names, dtype=str),
                "has_class_names": np.asarray(self.class_names is not None)}

    @classmethod
    def from_state_dict(cls, state: Dict[str, Any], device: Any = None) -> "ExampleBank":
        """The bank a ``state_dict`` was taken from: the prepared rows are copied back as they are, so scores have the same bits."""
        rows = np.asarray(state["rows"], dtype=np.float32)
        n_classes = int(state["n_classes"])
        names = [str(s) for s in np.asarray(state["class_names"]).reshape(-1).tolist()] if bool(np.asarray(state["has_class_names"])) else None
        bank = cls(int(state["dim"]), n_classes=None if n_classes < 0 else n_classes, metric=str(state["metric"]), device=device, class_names=names)
        if rows.ndim != 2 or rows.shape[1] != bank.dim:
            raise ValueError(f"rows of shape {rows.shape}: [n, {bank.dim}] expected")
        lab = bank._host_labels(np.asarray(state["labels"]), rows.shape[0])
        if rows.shape[0]:
            dev = bank.device
            with torch.cuda.device(dev):
                bank._append(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), False, lab)
        return bank


def detect_events_by_example(model: Any, bank: ExampleBank, sources: Sequence[Any], window_s: float, hop_s: Optional[float] = None, *, top_m: int = 1,
                             mode: str = "similarity", **detect_events_keywords) -> Dict[str, Any]:
    """:func:`avex_amd.detection.detect_events` with ``bank.scorer(top_m=top_m, mode=mode)`` as the probe: files to events from annotated
    examples.  ``detect_events_keywords``: the thresholds, the rules and the embedding arguments of ``detect_events``."""
    from . import detection
    return detection.detect_events(model, bank.scorer(top_m=top_m, mode=mode), sources, window_s, hop_s, **detect_events_keywords)
