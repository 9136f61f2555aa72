"""Call-type discovery: density clustering (DBSCAN) over window embeddings, for the question "what is in these recordings" when neither
the classes nor their number are known.

``dbscan(index_or_rows, eps, min_samples)`` gives every row a cluster number or ``-1`` (noise: in field recordings, most windows),
``k_distance(index, k)`` the curve one reads ``eps`` from.  The arithmetic runs in ``libavexhip.so`` (``csrc/density.hip``) on the fp32
MFMA tile the search uses; the ``N x N`` distance matrix is never stored (working memory is ``O(N)`` integers), and there is no CPU
fallback.

Semantics (the tests hold them; ``tests/_density_ref.py`` restates them in NumPy):

* **Prepared rows.**  ``metric="cosine"``: each row divided by ``max(||row||, 1e-12)`` in fp32 -- the rows an
  :class:`avex_amd.search.EmbeddingIndex` holds, prepared by the same code.  ``metric="euclidean"``: each row minus the fp32 column mean
  (the fp64 column sum over ``N``, rounded to fp32), as the k-means of :mod:`avex_amd.clustering` centres its rows.  The squared norm
  ``nx`` of a row is the diagonal of the same tile product that gives the similarities, so bit-identical rows are at distance exactly 0.
* **Distance**, in fp32, from the tile product ``s`` of two prepared rows: cosine ``min(max(1.0f - s, 0.0f), 2.0f)``; euclidean
  ``sqrtf(max((nx + ny) - 2 s, 0.0f))``.
* **Neighbour.**  ``j`` is a neighbour of ``i`` iff ``dist <= float32(eps)``; a row is always its own neighbour.  A row outside the
  graph -- its ``nx`` is not a finite number: the prepared row holds a NaN or an Inf -- is a neighbour of nobody: its count is 0, it is
  not core, its label is ``-1``, and ``nonfinite`` counts it.  (Centring spreads a NaN or an Inf to its whole column: with
  ``metric="euclidean"`` one such value puts every row outside.)
* **Symmetry.**  ``s(i, j)`` and ``s(j, i)`` are the same bits: both operands of the tile get the same k assignment and the same order
  of accumulation.  The neighbour relation is exactly symmetric, and the rest relies on it.
* **Counts and core rows.**  ``n_neighbors[i]``: the neighbours of ``i``, itself included (scikit-learn's convention);
  ``core[i] = n_neighbors[i] >= min_samples``.
* **Clusters.**  The connected components of the core rows under the neighbour relation, numbered ``0, 1, ..`` in the order of their
  lowest core row.  A row that is not core but has a core neighbour is a border row: it takes the smallest cluster number among its
  core neighbours.  Every other row gets ``-1``.  This is what ``sklearn.cluster.DBSCAN`` returns wherever no pair sits at the threshold.
* **Sizes and exemplars.**  ``sizes[c]``: the rows labelled ``c``; ``exemplar[c]``: the core row of ``c`` with the most neighbours, the
  lower row on a tie.
* **Independence.**  The result is a function of the rows alone: counts, labels and keys are integers and every atomic is an integer
  add, min or max.  It does not depend on ``batch_size``, on the index's ``chunk_rows``, on the pieces the rows were added in, or on
  the run.

:func:`dbscan` SYNCHRONISES with the device: components grow by rounds (per row the smallest label among its core neighbours, hooked
onto the row's root, then pointer jumping), each round is one ``O(N^2 D)`` pass, and the host reads one 4-byte "changed" word per
round -- and the number of clusters once at the end.  The round that changes nothing is the last; ``rounds`` counts them all.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _capi, search
from ._metric_inputs import _as_tensor, _stream
from .search import EmbeddingIndex, _shape2

DENSITY_METRICS = ("cosine", "euclidean")
_FLT_MAX = 3.4028234663852886e38
MAX_BLOCK = 1 << 22            # avexhip_density_max_block(): rows of one block of a launch

__all__ = ["dbscan", "k_distance", "DENSITY_METRICS"]


def _check_dbscan_args(eps, min_samples, metric, batch_size, max_rounds) -> None:
    """The argument checks that need no GPU."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not 0.0 <= float(eps) <= _FLT_MAX:
        raise ValueError(f"eps={eps!r}: a finite number >= 0 expected")
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or not 1 <= int(min_samples) <= search.MAX_ROWS:
        raise ValueError(f"min_samples={min_samples!r}: an integer >= 1 expected")
    if metric not in DENSITY_METRICS:
        raise ValueError(f"metric={metric!r}: one of {DENSITY_METRICS} expected")
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or int(batch_size) < 1:
        raise ValueError(f"batch_size={batch_size!r}: a positive integer expected")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or int(max_rounds) < 1:
        raise ValueError(f"max_rounds={max_rounds!r}: a positive integer expected")


def _index_chunks(index: EmbeddingIndex) -> List[Tuple[int, int, int]]:
    """(device address, first global row, rows) of every chunk of an index: the rows are used where they are."""
    n = len(index)
    return [(c.data_ptr(), i * index.chunk_rows, min(index.chunk_rows, n - i * index.chunk_rows)) for i, c in enumerate(index._chunks)]


def _blocks(chunks, rows_per_block: int, dpad: int) -> List[Tuple[int, int, int]]:
    out = []
    for ptr, r0, nc in chunks:
        for b in range(0, nc, rows_per_block):
            out.append((ptr + 4 * b * dpad, r0 + b, min(rows_per_block, nc - b)))
    return out


def dbscan(x, eps: float, min_samples: int = 5, *, metric: str = "cosine", batch_size: int = 65536, max_rounds: int = 10000,
           _timing: Optional[dict] = None) -> Dict[str, Any]:
    """DBSCAN of ``x``: ``[N, D]`` rows (NumPy or torch, any float dtype, host or device) or an :class:`EmbeddingIndex`, whose rows are
    used in place (a cosine index only: a ``"dot"`` index, and ``metric="euclidean"`` on an index, raise ``ValueError``).  Euclidean rows
    go through the centring pass of :mod:`avex_amd.clustering` and share its limit of 2^24 rows.

    Returns ``labels [N]`` int32, ``core [N]`` bool, ``n_neighbors [N]`` int32, ``sizes`` / ``exemplar [n_clusters]`` int32 (device
    tensors) and the host integers ``n_clusters``, ``rounds`` and ``nonfinite``; for an index also ``exemplar_recording``,
    ``exemplar_start_s`` and ``exemplar_end_s``, the exemplars' metadata.  See the module docstring for the semantics.  ``batch_size``:
    rows of one launch's row block; the result does not depend on it.  This function synchronises with the device once per round;
    more than ``max_rounds`` rounds raise :class:`avex_amd._capi.AvexHipError`.  ``_timing`` (a dict, for ``scripts/density_bench.py``)
    puts events around the count pass and around every round's hook pass and receives ``count_s`` and ``hook_s`` (one per round)."""
    _check_dbscan_args(eps, min_samples, metric, batch_size, max_rounds)
    index = x if isinstance(x, EmbeddingIndex) else None
    if index is not None:
        if index.metric != "cosine":
            raise ValueError(f"an index of metric {index.metric!r}: dbscan needs the normalised rows of a cosine index")
        if metric != "cosine":
            raise ValueError("metric='euclidean' on an index: its rows are already normalised; pass the embeddings themselves")
        if len(index) == 0:
            raise ValueError("the index is empty")
    else:
        shape = _shape2(x)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"x of shape {shape}: [N, D] rows with N, D >= 1 expected")
        if shape[0] > search.MAX_ROWS:
            raise ValueError(f"{shape[0]} rows: more than 2^31 - 1")
    _capi.require_gpu()
    lib = _capi.lib()
    keep = None                                   # whatever owns the prepared rows, alive until the last launch is queued
    if index is not None:
        dev = index.device
    else:
        t = _as_tensor(x)
        dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        if index is not None:
            n, dpad, chunks = len(index), index.dpad, _index_chunks(index)
        elif metric == "cosine":
            keep = EmbeddingIndex(int(shape[1]), metric="cosine", device=dev)
            keep.add(x)
            n, dpad, chunks = len(keep), keep.dpad, _index_chunks(keep)
        else:
            from .clustering import _Prepared, _embeddings
            keep = _Prepared(_embeddings(x, dev), 1, 1, 1e-4)
            ptr, dpad = keep.centred_rows()
            n, chunks = keep.n, [(ptr, 0, keep.n)]
        s = _stream()
        row_blocks = _blocks(chunks, min(int(batch_size), MAX_BLOCK), dpad)
        col_blocks = _blocks(chunks, MAX_BLOCK, dpad)
        ws_bytes = int(lib.avexhip_density_workspace_bytes(n))
        if ws_bytes == 0:
            raise _capi.AvexHipError(f"density: no workspace for {n} rows")
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        a = _capi.DensityArgs()
        a.n, a.dpad, a.metric = n, dpad, 1 if metric == "cosine" else 0      # AVEXHIP_DENSITY_COSINE / _EUCLIDEAN
        a.eps, a.min_samples = float(np.float32(eps)), int(min_samples)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        ref = C.byref(a)

        marks = []

        def pairs(fn, what):
            if _timing is not None:
                marks.append([torch.cuda.Event(enable_timing=True) for _ in range(2)])
                marks[-1][0].record()
            for a.rows, a.row0, a.n_rows in row_blocks:
                for a.cols, a.col0, a.n_cols in col_blocks:
                    _capi.check(fn(ref, s), what)
            if _timing is not None:
                marks[-1][1].record()

        _capi.check(lib.avexhip_density_begin(ref, s), "density_begin")
        for a.rows, a.row0, a.n_rows in col_blocks:
            _capi.check(lib.avexhip_density_norms(ref, s), "density_norms")
        pairs(lib.avexhip_density_count, "density_count")
        _capi.check(lib.avexhip_density_core(ref, s), "density_core")
        changed = torch.zeros((1,), dtype=torch.int32, device=dev)
        rounds = 0
        while True:
            if rounds >= int(max_rounds):
                raise _capi.AvexHipError(f"dbscan: the components had not settled after max_rounds={max_rounds} rounds")
            _capi.check(lib.avexhip_density_round_begin(ref, s), "density_round_begin")
            pairs(lib.avexhip_density_hook, "density_hook")
            _capi.check(lib.avexhip_density_round_end(ref, changed.data_ptr(), s), "density_round_end")
            rounds += 1
            if int(changed.item()) == 0:          # the 4-byte read of this round
                break
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        core = torch.empty((n,), dtype=torch.bool, device=dev)
        n_neighbors = torch.empty((n,), dtype=torch.int32, device=dev)
        summary = torch.zeros((2,), dtype=torch.int32, device=dev)
        _capi.check(lib.avexhip_density_labels(ref, labels.data_ptr(), core.data_ptr(), n_neighbors.data_ptr(), summary.data_ptr(), s), "density_labels")
        n_clusters, nonfinite = (int(v) for v in summary.cpu().tolist())
        if _timing is not None:
            times = [e[0].elapsed_time(e[1]) * 1e-3 for e in marks]
            _timing["count_s"], _timing["hook_s"] = times[0], times[1:]
        sizes = torch.empty((n_clusters,), dtype=torch.int32, device=dev)
        exemplar = torch.empty((n_clusters,), dtype=torch.int32, device=dev)
        if n_clusters:
            _capi.check(lib.avexhip_density_summary(ref, labels.data_ptr(), n_clusters, sizes.data_ptr(), exemplar.data_ptr(), s), "density_summary")
        out = {"labels": labels, "core": core, "n_neighbors": n_neighbors, "sizes": sizes, "exemplar": exemplar, "n_clusters": n_clusters,
               "rounds": rounds, "nonfinite": nonfinite}
        if index is not None and index._rec is not None:
            at = exemplar.to(torch.int64)
            out["exemplar_recording"], out["exemplar_start_s"], out["exemplar_end_s"] = index._rec[at], index._start[at], index._end[at]
        del keep
    return out


def k_distance(index: EmbeddingIndex, k: int, *, batch_size: int = 1024) -> torch.Tensor:
    """The cosine distance ``min(max(1 - s, 0), 2)`` of every row of a cosine index to its ``k``-th nearest OTHER row, as an ``[N]`` fp32
    device tensor (``inf`` where the index holds fewer than ``k`` other rows that give a number).  Sorted, it is the curve whose knee one
    reads ``eps`` from.  A row counts itself among its neighbours, so ``k`` here corresponds to ``min_samples = k + 1``: a row is core for
    ``dbscan(index, eps, k + 1)`` iff its ``k``-distance is ``<= eps``.  Built on :meth:`EmbeddingIndex.search_rows` (``exclude=None``):
    the similarities are the search's, ``1 <= k <= search.MAX_K``."""
    if not isinstance(index, EmbeddingIndex):
        raise ValueError("k_distance takes an EmbeddingIndex")
    if index.metric != "cosine":
        raise ValueError(f"an index of metric {index.metric!r}: k_distance is a cosine distance")
    search._check_search_args(k, None, 1, None, batch_size)
    n = len(index)
    if n == 0:
        raise ValueError("the index is empty")
    dev = index.device
    with torch.cuda.device(dev):
        out = torch.empty((n,), dtype=torch.float32, device=dev)
        step = 65536
        for r0 in range(0, n, step):
            rows = torch.arange(r0, min(r0 + step, n), dtype=torch.int64, device=dev)
            res = index.search_rows(rows, int(k), exclude=None, batch_size=int(batch_size))
            d = (1.0 - res["scores"][:, int(k) - 1]).clamp(0.0, 2.0)
            out[r0:r0 + step] = torch.where(res["count"] >= int(k), d, torch.full_like(d, float("inf")))
    return out
