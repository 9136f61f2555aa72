"""Clustering metrics on the device: seeded k-means, then ARI / NMI / V-measure against the ground-truth labels.

Reference: ``avex/evaluation/clustering.py`` (called from ``run_evaluate.py:962-970`` on the cached test embeddings and from
``training/clustering_evaluator.py``), which runs ``sklearn.cluster.KMeans(n_clusters, random_state=42, n_init=10, max_iter=300)`` and
three ``sklearn.metrics`` scores on the host.  ``eval_clustering`` and ``eval_clustering_multiple_k`` keep the reference's names,
argument names, defaults, return keys and ``ValueError`` text; embeddings and labels may be NumPy arrays or torch tensors, on the host
or on the device -- a device tensor is never copied to the host -- and the results are Python floats.  The arithmetic runs in
``libavexhip.so`` (``csrc/clustering.hip``); there is no CPU fallback.

The result is meant to be scikit-learn's *partition*, not an approximation of its scores: k-means is seeded, and everything KMeans
takes from its ``RandomState`` is independent of the data (per restart one weighted ``choice`` and ``2 + int(ln k)`` uniforms per
further centre), so the host draws those numbers up front and the device does everything that touches the data.  The three scores are
invariant under renaming clusters.  What is computed, and where it differs from the reference in the letter:

* **Embeddings in fp64 (or f16 / bf16) are converted to fp32 on the device and computed in fp32**; scikit-learn computes in the dtype
  it is given.  Distances of the assign step are ``||c||^2 - 2 x.c`` with fp32 operands on the fp32 MFMA (as scikit-learn's fp32 GEMM);
  centre sums add a cluster's rows in ascending row order, so a run is bit-reproducible; potentials, prefix sums, the tolerance, inertia
  and the scores are fp64.  The last bits of a distance differ from scikit-learn's, so a point that is equidistant from two centres
  to within fp32 rounding can fall on the other side; the goldens are sets whose partition survives such noise.
* All ``n_init`` restarts advance in lock-step (one launch per stage over all of them); a restart that has stopped is frozen.  The
  winner is the first restart with the strictly smallest inertia (scikit-learn also skips a better restart that is the same clustering,
  which cannot change the partition).
* Empty clusters are refilled as scikit-learn does: the ``e`` points farthest from their assigned centre, largest first (lower index
  on exact ties), become the ``e`` empty clusters in ascending id.
* Anything scikit-learn would raise on is swallowed into the all-zero dict, as the reference's ``except Exception`` does: in practice
  NaN or infinite embeddings, found by a flag of the centring pass that is read back with the results.
* Limits: ``n_clusters <= MAX_K`` (4096), ``n_init <= MAX_INIT`` (64), ``N <= MAX_N`` (2^24); beyond them ``ValueError``.

``silhouette_samples`` / ``silhouette_score`` are scikit-learn's functions of those names (metric ``"euclidean"`` or ``"cosine"``) on the
device: the metric the reference dropped "for speed" (clustering.py:123) while its configs still list ``clustering_silhouette``.
``eval_clustering_silhouette`` / ``eval_clustering_multiple_k_silhouette`` are the two reference functions with that column added; the
reference's own two keep their signatures and return values.

``kmeans`` and ``clustering_scores`` are the layers below.  Sharding the points over ranks is not built; the per-cluster sums and
counts of the update step are where an all-reduce would go.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Optional

import numpy as np
import torch

from . import _capi
from ._metric_inputs import _as_tensor, _device_of, _joint_ids, _len0, _stream

logger = logging.getLogger(__name__)

MAX_K = 4096                   # avexhip_clustering_max_k()
MAX_INIT = 64
MAX_N = 1 << 24
_POLL_EVERY = 8                # Lloyd iterations enqueued between two looks at the "restarts not finished" word

MAX_SIL_N = 1 << 19            # avexhip_silhouette_max_n()
MAX_SIL_LABELS = 4096          # avexhip_silhouette_max_labels()
_SIL_METRICS = {"euclidean": 0, "cosine": 1}      # AVEXHIP_SILHOUETTE_*

__all__ = ["eval_clustering", "eval_clustering_multiple_k", "kmeans", "clustering_scores", "MAX_K", "silhouette_samples", "silhouette_score",
           "eval_clustering_silhouette", "eval_clustering_multiple_k_silhouette"]


def _get_empty_clustering_metrics() -> Dict[str, float]:
    return {"clustering_ari": 0.0, "clustering_nmi": 0.0, "clustering_v_measure": 0.0}


def _get_empty_clustering_best_metrics() -> Dict[str, float]:
    return {"clustering_best_k": 0.0, "clustering_ari_best": 0.0, "clustering_nmi_best": 0.0, "clustering_v_measure_best": 0.0}


def _numel(x) -> int:
    return int(x.numel()) if isinstance(x, torch.Tensor) else int(np.asarray(x).size)


def _trials(k: int) -> int:
    return 2 + int(np.log(k))


def _draws(n: int, k: int, n_init: int, random_state):
    """Everything KMeans.fit takes from its RandomState, in stream order (none of it depends on the data): per restart the first
    centre -- ``choice`` over the uniform fp32 sample weights, called as is -- and ``2 + int(ln k)`` uniforms for each further centre."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    t = _trials(k)
    first = np.zeros(n_init, dtype=np.int32)
    u = np.zeros((n_init, max(k - 1, 0), t), dtype=np.float64)
    w = np.ones(n, dtype=np.float32)
    p = w / w.sum()
    for r in range(n_init):
        first[r] = rs.choice(n, p=p)
        for c in range(k - 1):
            u[r, c] = rs.uniform(size=t)
    return first, u


def _embeddings(x, dev: torch.device) -> torch.Tensor:
    t = _as_tensor(x)
    if t.dim() != 2:
        raise ValueError("embeddings must be 2-D (N, D)")
    t = t.to(dev).to(torch.float32)
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()      # a row-strided view is read in place


class _Prepared:
    """Centred embeddings in a workspace sized for clusterings of up to ``k_max`` clusters: prepare once, cluster for several k."""

    def __init__(self, x: torch.Tensor, k_max: int, n_init: int, tol: float):
        n, d = int(x.shape[0]), int(x.shape[1])
        if n > MAX_N:
            raise ValueError(f"{n} points exceed the clustering kernels' limit of {MAX_N}")
        if d == 0:
            raise ValueError("embeddings must have a non-zero width")
        self.x, self.n, self.d, self.n_init, self.tol, self.k_max = x, n, d, n_init, float(tol), k_max
        self.lib = _capi.lib()
        self.bytes = int(self.lib.avexhip_clustering_workspace_bytes(n, d, k_max, n_init))
        if self.bytes == 0:
            raise ValueError(f"clustering workspace: unsupported shape (n {n}, d {d}, k {k_max}, n_init {n_init})")
        self.ws = torch.empty((self.bytes,), dtype=torch.uint8, device=x.device)
        _capi.check(self.lib.avexhip_clustering_prepare(C.byref(self.args(k_max, 1)), _stream()), "clustering_prepare")

    def args(self, k: int, max_iter: int) -> _capi.ClusteringArgs:
        a = _capi.ClusteringArgs()
        a.x, a.ld_x, a.n, a.d, a.k, a.n_init, a.max_iter, a.tol = self.x.data_ptr(), self.x.stride(0), self.n, self.d, k, self.n_init, max_iter, self.tol
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.bytes
        return a

    def centred_rows(self):
        """(device address, row stride in floats) of X - mean as the centring pass left it."""
        ptr = self.lib.avexhip_clustering_centred_rows(C.byref(self.args(self.k_max, 1)))
        if not ptr:
            raise _capi.AvexHipError("clustering workspace holds no centred rows")
        return int(ptr), (self.d + 31) // 32 * 32


def _check_kmeans_args(n: int, n_clusters: int, n_init: int, max_iter: int) -> None:
    if n_clusters < 1:
        raise ValueError("n_clusters must be >= 1")
    if n_clusters > MAX_K:
        raise ValueError(f"n_clusters = {n_clusters} exceeds the clustering kernels' limit of {MAX_K}")
    if n_clusters > n:
        raise ValueError(f"n_samples={n} should be >= n_clusters={n_clusters}.")
    if not 1 <= n_init <= MAX_INIT:
        raise ValueError(f"n_init = {n_init} outside [1, {MAX_INIT}]")
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")


def _run(prep: _Prepared, k: int, max_iter: int, random_state, init: Optional[torch.Tensor], _timing: Optional[dict] = None) -> Dict[str, object]:
    lib, dev, n, d, R = prep.lib, prep.x.device, prep.n, prep.d, prep.n_init
    s = _stream()
    a = prep.args(k, max_iter)
    ev = []

    def mark():
        if _timing is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

    mark()
    if init is None:
        first, u = _draws(n, k, R, random_state)
        first_d = torch.from_numpy(first).to(dev)
        u_d = torch.from_numpy(u.reshape(-1) if u.size else np.zeros(1)).to(dev)
        _capi.check(lib.avexhip_clustering_seed(C.byref(a), first_d.data_ptr(), u_d.data_ptr(), s), "clustering_seed")
    else:
        _capi.check(lib.avexhip_clustering_set_init(C.byref(a), init.data_ptr(), init.stride(0), s), "clustering_set_init")
    mark()
    unfinished = torch.ones((1,), dtype=torch.int32, device=dev)
    done_iters, split = 0, []
    while done_iters <= max_iter:                  # at most max_iter updates and one closing assign
        if _timing is None:
            _capi.check(lib.avexhip_clustering_iterate(C.byref(a), _POLL_EVERY, 0, unfinished.data_ptr(), s), "clustering_iterate")
        else:                                      # the assign product and the rest launched separately, with events between them
            for _ in range(_POLL_EVERY):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                for stage in (1, 2):
                    _capi.check(lib.avexhip_clustering_iterate(C.byref(a), 1, stage, unfinished.data_ptr(), s), "clustering_iterate")
                    e[stage].record()
                split.append(e)
        done_iters += _POLL_EVERY
        if int(unfinished.item()) == 0:            # the poll: one word every _POLL_EVERY iterations
            break
    mark()
    out = {"labels": torch.empty((n,), dtype=torch.int32, device=dev), "centers": torch.empty((k, d), dtype=torch.float32, device=dev),
           "inertias": torch.empty((R,), dtype=torch.float64, device=dev), "n_iters": torch.empty((R,), dtype=torch.int32, device=dev),
           "seed_indices": torch.empty((R, k), dtype=torch.int32, device=dev)}
    summary = torch.empty((4,), dtype=torch.int32, device=dev)
    a.labels_out, a.centers_out, a.inertias_out = out["labels"].data_ptr(), out["centers"].data_ptr(), out["inertias"].data_ptr()
    a.n_iters_out, a.seeds_out, a.summary_out = out["n_iters"].data_ptr(), out["seed_indices"].data_ptr(), summary.data_ptr()
    _capi.check(lib.avexhip_clustering_finish(C.byref(a), s), "clustering_finish")
    mark()
    out["_summary"] = summary
    if _timing is not None:
        torch.cuda.synchronize(dev)
        _timing["seeding_s"] = _timing.get("seeding_s", 0.0) + ev[0].elapsed_time(ev[1]) * 1e-3
        _timing["assign_s"] = _timing.get("assign_s", 0.0) + sum(e[0].elapsed_time(e[1]) for e in split) * 1e-3
        _timing["update_s"] = _timing.get("update_s", 0.0) + sum(e[1].elapsed_time(e[2]) for e in split) * 1e-3
        _timing["finish_s"] = _timing.get("finish_s", 0.0) + ev[2].elapsed_time(ev[3]) * 1e-3
        _timing["iterations_enqueued"] = _timing.get("iterations_enqueued", 0) + len(split)
    return out


def kmeans(x, n_clusters: int, *, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4, random_state=42, init=None,
           _timing: Optional[dict] = None) -> Dict[str, object]:
    """scikit-learn's ``KMeans(n_clusters, init="k-means++", n_init, max_iter, tol, random_state, algorithm="lloyd").fit(x)`` on the device.

    Returns device tensors ``labels`` (int32 ``[N]``), ``centers`` (fp32 ``[k, D]``, the mean added back), per restart ``inertias``
    (fp64), ``n_iters`` and ``seed_indices`` (``[n_init, k]``, the data rows k-means++ chose; -1 with ``init``), and the scalars
    ``inertia``, ``n_iter`` (as scikit-learn counts), ``best_init`` and ``finite`` (False: the input held a NaN or an infinity and the
    rest is meaningless).  ``init`` = an explicit ``[k, D]`` array means one run from those centres.  Inputs in fp64 are computed in fp32.
    """
    n_clusters, max_iter = int(n_clusters), int(max_iter)
    t = _as_tensor(x)
    if t.dim() != 2:
        raise ValueError("embeddings must be 2-D (N, D)")
    n_init = 1 if init is not None else int(n_init)
    _check_kmeans_args(int(t.shape[0]), n_clusters, n_init, max_iter)
    _capi.require_gpu()
    dev = _device_of(x, init)
    with torch.cuda.device(dev):
        xd = _embeddings(x, dev)
        init_d = None
        if init is not None:
            init_d = _as_tensor(init).to(dev).to(torch.float32).contiguous()
            if tuple(init_d.shape) != (n_clusters, xd.shape[1]):
                raise ValueError(f"The shape of the initial centers {tuple(init_d.shape)} does not match the number of clusters "
                                 f"{n_clusters} and features {int(xd.shape[1])}.")
        prep = _Prepared(xd, n_clusters, n_init, tol)
        out = _run(prep, n_clusters, max_iter, random_state, init_d, _timing)
        host = out.pop("_summary").cpu()                     # the one read-back beside the polls
        best = int(host[0])
        out.update({"inertia": float(out["inertias"][best]), "n_iter": int(host[1]), "best_init": best, "finite": bool(host[2])})
        return out


def _dense_ids(a: torch.Tensor, dev: torch.device):
    ids = _joint_ids(a.reshape(-1), None, dev)[0]
    return ids, (int(ids.max()) + 1 if ids.numel() else 0)


def _scores_launch(true_ids: torch.Tensor, n_true: int, pred_ids: torch.Tensor, n_pred: int, out: torch.Tensor) -> None:
    lib = _capi.lib()
    nbytes = int(lib.avexhip_clustering_scores_workspace_bytes(n_true, n_pred))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=out.device)
    _capi.check(lib.avexhip_clustering_scores(true_ids.data_ptr(), n_true, pred_ids.data_ptr(), n_pred, int(true_ids.numel()), ws.data_ptr(),
                                              nbytes, out.data_ptr(), _stream()), "clustering_scores")


def clustering_scores(labels_true, labels_pred) -> Dict[str, float]:
    """``{"ari", "nmi", "v_measure"}`` of two integer label vectors (any integers): ``adjusted_rand_score``,
    ``normalized_mutual_info_score`` (arithmetic mean) and ``v_measure_score`` (beta 1) from an integer contingency table, in fp64."""
    a, b = _as_tensor(labels_true), _as_tensor(labels_pred)
    if a.dim() != 1 or b.dim() != 1 or a.shape[0] != b.shape[0]:
        raise ValueError("labels_true and labels_pred must be 1-D and of the same length")
    if a.shape[0] == 0:
        raise ValueError("labels must not be empty")
    _capi.require_gpu()
    dev = _device_of(labels_true, labels_pred)
    with torch.cuda.device(dev):
        ia, na = _dense_ids(a, dev)
        ib, nb = _dense_ids(b, dev)
        out = torch.empty((3,), dtype=torch.float64, device=dev)
        _scores_launch(ia, na, ib, nb, out)
        h = out.cpu()
        return {"ari": float(h[0]), "nmi": float(h[1]), "v_measure": float(h[2])}


def _check_random_state(seed) -> np.random.RandomState:
    """sklearn.utils.check_random_state."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def _label_tensor(labels) -> torch.Tensor:
    """1-D labels as a tensor where they live; a non-numeric NumPy dtype (strings, objects) is numbered on the host first."""
    if not isinstance(labels, torch.Tensor):
        a = np.asarray(labels)
        if a.dtype.kind not in "biuf":
            labels = np.unique(a.reshape(-1), return_inverse=True)[1].astype(np.int64).reshape(a.shape)
    t = _as_tensor(labels)
    if t.dim() != 1:
        raise ValueError(f"y should be a 1d array, got an array of shape {tuple(t.shape)} instead.")
    return t


def _sil_layout(ids: torch.Tensor, n_labels: int, dev: torch.device):
    """The cluster-ordered layout of avexhip_silhouette_args: rows in label order (stable: ascending row inside a cluster), every cluster
    padded to a multiple of 32 slots, the whole to a multiple of 128.  -> slot_src, group_label, counts (int32, device), n_slots."""
    n = int(ids.numel())
    ids64 = ids.to(torch.int64)
    counts = torch.bincount(ids64, minlength=n_labels)
    counts_h = counts.cpu().numpy()
    padded = (counts_h + 31) // 32 * 32
    offset = np.concatenate([[0], np.cumsum(padded)])
    n_slots = int((offset[-1] + 127) // 128 * 128)
    start = np.cumsum(counts_h) - counts_h
    shift = torch.from_numpy((offset[:-1] - start).astype(np.int64)).to(dev)
    order = torch.argsort(ids64, stable=True)
    slot = torch.arange(n, device=dev, dtype=torch.int64) + shift[ids64[order]]
    slot_src = torch.full((n_slots,), -1, dtype=torch.int32, device=dev)
    slot_src[slot] = order.to(torch.int32)
    group = np.full(n_slots // 32, -1, dtype=np.int32)
    group[: int(offset[-1]) // 32] = np.repeat(np.arange(n_labels, dtype=np.int32), padded // 32)
    return slot_src, torch.from_numpy(group).to(dev), counts.to(torch.int32).contiguous(), n_slots


def _sil_launch(rows_ptr: int, ld: int, n: int, d: int, ids: torch.Tensor, n_labels: int, metric: str, batch_size: int, dev: torch.device,
                _timing: Optional[dict] = None):
    """-> (samples [n] fp64, summary [2] fp64 = mean, finite flag), both on the device; nothing is read back here but the cluster sizes."""
    lib = _capi.lib()
    slot_src, group, counts, n_slots = _sil_layout(ids, n_labels, dev)
    batch = min(max(int(batch_size), 1), n_slots)
    nbytes = int(lib.avexhip_silhouette_workspace_bytes(n_slots, d, n_labels, batch))
    if nbytes == 0:
        raise ValueError(f"silhouette workspace: unsupported shape (n {n}, d {d}, labels {n_labels}, batch {batch})")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    samples = torch.zeros((n,), dtype=torch.float64, device=dev)
    summary = torch.empty((2,), dtype=torch.float64, device=dev)
    a = _capi.SilhouetteArgs()
    a.x, a.ld_x, a.n, a.d, a.metric, a.n_labels, a.n_slots, a.batch = rows_ptr, ld, n, d, _SIL_METRICS[metric], n_labels, n_slots, batch
    a.slot_src, a.group_label, a.counts = slot_src.data_ptr(), group.data_ptr(), counts.data_ptr()
    a.workspace, a.workspace_bytes, a.samples_out = ws.data_ptr(), nbytes, samples.data_ptr()
    s = _stream()
    ev = []

    def mark():
        if _timing is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

    mark()
    _capi.check(lib.avexhip_silhouette_prepare(C.byref(a), s), "silhouette_prepare")
    mark()
    for row0 in range(0, n_slots, batch):
        a.row0, a.nb = row0, min(batch, n_slots - row0)
        for stage in ((0,) if _timing is None else (1, 2)):      # timed: the product and the per-point pass launched apart
            a.stages = stage
            _capi.check(lib.avexhip_silhouette_batch(C.byref(a), s), "silhouette_batch")
            mark()
    _capi.check(lib.avexhip_silhouette_finalize(C.byref(a), summary.data_ptr(), s), "silhouette_finalize")
    mark()
    if _timing is not None:
        torch.cuda.synchronize(dev)
        dt = [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(len(ev) - 1)]
        _timing["prepare_s"] = _timing.get("prepare_s", 0.0) + dt[0]
        _timing["product_s"] = _timing.get("product_s", 0.0) + sum(dt[1:-1:2])
        _timing["finalize_s"] = _timing.get("finalize_s", 0.0) + sum(dt[2:-1:2]) + dt[-1]
        _timing["n_slots"] = n_slots
    return samples, summary


def _silhouette(X, labels, metric, sample_size, random_state, batch_size, _timing=None):
    if metric not in _SIL_METRICS:
        raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
    t = _as_tensor(X)
    if t.dim() != 2:
        raise ValueError(f"Expected 2D array, got {t.dim()}D array instead")
    lab = _label_tensor(labels)
    if int(t.shape[0]) != int(lab.shape[0]):
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{int(t.shape[0])}, {int(lab.shape[0])}]")
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    idx = None
    if sample_size is not None:
        idx = _check_random_state(random_state).permutation(int(t.shape[0]))[: int(sample_size)]      # scikit-learn's draw, on the host
    n = int(t.shape[0]) if idx is None else int(idx.shape[0])
    if n > MAX_SIL_N:
        raise ValueError(f"{n} points exceed the silhouette kernels' limit of {MAX_SIL_N}")
    if n > 0 and int(t.shape[1]) == 0:
        raise ValueError("X must have a non-zero width")
    _capi.require_gpu()
    dev = _device_of(X, labels)
    with torch.cuda.device(dev):
        xd, lab = _embeddings(X, dev), lab.to(dev)
        if idx is not None:                        # rows and labels gathered on the device
            idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
            xd, lab = xd[idx_d].contiguous(), lab[idx_d]
        ids, n_labels = _dense_ids(lab, dev)
        if not 1 < n_labels < n:
            raise ValueError(f"Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)")
        if n_labels > MAX_SIL_LABELS:
            raise ValueError(f"{n_labels} labels exceed the silhouette kernels' limit of {MAX_SIL_LABELS}")
        if metric == "euclidean":                  # distances do not change under translation; the fp32 Gram form needs small norms
            prep = _Prepared(xd, 1, 1, 1e-4)
            ptr, ld = prep.centred_rows()
        else:
            ptr, ld = xd.data_ptr(), xd.stride(0)
        samples, summary = _sil_launch(ptr, ld, n, int(xd.shape[1]), ids, n_labels, metric, batch_size, dev, _timing)
        host = summary.cpu()                       # the mean and the finite flag in one read-back
        if not bool(host[1]):
            raise ValueError("Input X contains NaN or infinity.")
        return samples, float(host[0])


def silhouette_samples(X, labels, *, metric: str = "euclidean", batch_size: int = 2048) -> torch.Tensor:
    """scikit-learn's ``silhouette_samples(X, labels, metric=...)`` on the device: an ``[N]`` fp64 device tensor.

    ``X`` (NumPy or torch, host or device, any float dtype) is computed in fp32; ``labels`` are any integers or a non-numeric NumPy
    dtype.  ``metric="euclidean"`` is ``sqrt(max(||x||^2 + ||y||^2 - 2 x.y, 0))`` on the centred rows, ``"cosine"`` is
    ``clip(1 - x^.y^, 0, 2)`` on rows divided by ``max(||row||, 1e-12)``; anything else raises.  ``a`` is the mean distance to the other
    members of the point's cluster, ``b`` the smallest mean distance to another cluster, ``s = (b - a) / max(a, b)``; a point alone in
    its cluster gets 0.  ``batch_size`` rows of the cluster-ordered layout are handled per launch (working memory
    ``O(N D + batch_size n_labels)``); the result is the same bit for bit for every ``batch_size`` and from run to run."""
    return _silhouette(X, labels, metric, None, None, batch_size)[0]


def silhouette_score(X, labels, *, metric: str = "euclidean", sample_size: Optional[int] = None, random_state=None, batch_size: int = 2048,
                     _timing: Optional[dict] = None) -> float:
    """scikit-learn's ``silhouette_score``: the mean of ``silhouette_samples`` (an fp64 sum in a fixed order), as a Python float.
    ``sample_size``: the subsample ``check_random_state(random_state).permutation(N)[:sample_size]``, drawn on the host as scikit-learn
    draws it; the number of labels is checked on the subsample."""
    return _silhouette(X, labels, metric, sample_size, random_state, batch_size, _timing)[1]


def _reduce_labels(labels) -> torch.Tensor:
    """clustering.py:66-72: [N, 1] squeezed, wider label matrices reduced by argmax."""
    lab = _as_tensor(labels)
    if lab.dim() > 1:
        lab = lab.squeeze() if lab.shape[1] == 1 else lab.argmax(dim=1)
    return lab.reshape(-1)


def _eval_prepared(prep: _Prepared, true_ids: torch.Tensor, n_true: int, k: int, random_state, silhouette: bool = False) -> Dict[str, float]:
    dev = prep.x.device
    run = _run(prep, k, 300, random_state, None)
    out = torch.empty((3,), dtype=torch.float64, device=dev)
    _scores_launch(true_ids, n_true, run["labels"], k, out)
    sil = torch.zeros((2,), dtype=torch.float64, device=dev)
    if silhouette:                                 # of the partition just computed, on the rows the centring pass left
        ids, n_ids = _dense_ids(run["labels"], dev)
        if 2 <= n_ids <= prep.n - 1 and n_ids <= MAX_SIL_LABELS and prep.n <= MAX_SIL_N:
            ptr, ld = prep.centred_rows()
            sil = _sil_launch(ptr, ld, prep.n, prep.d, ids, n_ids, "euclidean", 2048, dev)[1]
    host = torch.cat([out, run["_summary"].to(torch.float64), sil]).cpu()      # the scores and the finite flag in one read-back
    extra = {"clustering_silhouette": 0.0} if silhouette else {}
    if not bool(host[3 + 2]):
        logger.error("Clustering evaluation failed: Input X contains NaN or infinity.")
        return {**_get_empty_clustering_metrics(), **extra}
    if silhouette:
        extra["clustering_silhouette"] = float(host[7])
    return {"clustering_ari": float(host[0]), "clustering_nmi": float(host[1]), "clustering_v_measure": float(host[2]), **extra}


def eval_clustering(embeds, labels, n_clusters: Optional[int] = None, random_state: int = 42) -> Dict[str, float]:
    """``{"clustering_ari", "clustering_nmi", "clustering_v_measure"}`` of a k-means clustering of the embeddings against the labels
    (clustering.py:20-111).  ``n_clusters=None``: the number of distinct labels ``>= 0``; fewer than 2 clusters, NaN / infinite
    embeddings, or empty inputs give the all-zero dict; ``n_clusters > N`` is clipped to ``N``."""
    if _numel(embeds) == 0 or _numel(labels) == 0:
        logger.warning("Empty embeddings or labels provided to clustering evaluation")
        return _get_empty_clustering_metrics()
    if _len0(embeds) != _len0(labels):
        raise ValueError(f"Embeddings and labels must have same length: {_len0(embeds)} vs {_len0(labels)}")
    return _eval(embeds, labels, [n_clusters], random_state)[0][1]


def eval_clustering_silhouette(embeds, labels, n_clusters: Optional[int] = None, random_state: int = 42) -> Dict[str, float]:
    """``eval_clustering`` with one more key, ``"clustering_silhouette"``: the Euclidean silhouette score of the k-means partition it
    computes, on the same centred data (the column the reference's configs ask for and its code no longer fills).  0.0 wherever
    ``eval_clustering`` returns the all-zero dict."""
    empty = {**_get_empty_clustering_metrics(), "clustering_silhouette": 0.0}
    if _numel(embeds) == 0 or _numel(labels) == 0:
        logger.warning("Empty embeddings or labels provided to clustering evaluation")
        return empty
    if _len0(embeds) != _len0(labels):
        raise ValueError(f"Embeddings and labels must have same length: {_len0(embeds)} vs {_len0(labels)}")
    return _eval(embeds, labels, [n_clusters], random_state, silhouette=True)[0][1]


def _eval(embeds, labels, ks, random_state, silhouette: bool = False):
    """[(k, metrics)] for every k in ks (None = the number of distinct labels >= 0): the data is centred and uploaded once."""
    n = _len0(embeds)
    zero = {**_get_empty_clustering_metrics(), **({"clustering_silhouette": 0.0} if silhouette else {})}
    if _as_tensor(embeds).dim() != 2:
        return [(k, dict(zero)) for k in ks]      # scikit-learn raises on anything but a 2-D array: swallowed
    _capi.require_gpu()
    dev = _device_of(embeds, labels)
    with torch.cuda.device(dev):
        lab = _reduce_labels(labels).to(dev)
        true_ids, n_true = _dense_ids(lab, dev)
        resolved = []
        for k in ks:
            if k is None:
                k = int((torch.unique(lab) >= 0).sum())
            k = int(k)
            if k > n:
                logger.warning(f"Number of clusters ({k}) cannot exceed number of samples ({n})")
                k = n
            resolved.append(k)
        valid = [k for k in resolved if k >= 2]
        if valid and max(valid) > MAX_K:
            raise ValueError(f"n_clusters = {max(valid)} exceeds the clustering kernels' limit of {MAX_K}")
        prep = _Prepared(_embeddings(embeds, dev), max(valid), 10, 1e-4) if valid else None
        res = []
        for k in resolved:
            if k < 2:
                logger.warning(f"Need at least 2 clusters for meaningful clustering evaluation, got {k}")
                res.append((k, dict(zero)))
            else:
                res.append((k, _eval_prepared(prep, true_ids, n_true, k, random_state, silhouette)))
        return res


def eval_clustering_multiple_k(embeds, labels, k_range: Optional[tuple] = None, random_state: int = 42) -> Dict[str, float]:
    """The best of ``eval_clustering`` over a range of k, by ARI, the first on ties (clustering.py:114-190): ``{"clustering_best_k",
    "clustering_ari_best", "clustering_nmi_best", "clustering_v_measure_best"}``.  Default range: ``max(2, true_k - 2) ..
    min(N // 2, true_k + 3)``; the range stops at ``k >= N``.  The data is centred and uploaded once."""
    return _eval_multiple_k(embeds, labels, k_range, random_state, False)


def eval_clustering_multiple_k_silhouette(embeds, labels, k_range: Optional[tuple] = None, random_state: int = 42) -> Dict[str, float]:
    """``eval_clustering_multiple_k`` with one more key, ``"clustering_silhouette_best"``: the Euclidean silhouette score at the k its
    (unchanged) ARI rule selects; 0.0 wherever it returns the all-zero dict."""
    return _eval_multiple_k(embeds, labels, k_range, random_state, True)


def _eval_multiple_k(embeds, labels, k_range, random_state, silhouette: bool) -> Dict[str, float]:
    """``eval_clustering_multiple_k``; with ``silhouette`` each k also carries its silhouette score and the winner's is reported."""
    empty = {**_get_empty_clustering_best_metrics(), **({"clustering_silhouette_best": 0.0} if silhouette else {})}
    if _numel(embeds) == 0 or _numel(labels) == 0:
        logger.warning("Empty embeddings or labels provided to clustering evaluation")
        return empty
    n = _len0(embeds)
    if k_range is None:
        lab = _reduce_labels(labels)
        true_k = int((torch.unique(lab) >= 0).sum())
        k_range = (max(2, true_k - 2), min(n // 2, true_k + 3))
    ks = [k for k in range(int(k_range[0]), int(k_range[1]) + 1) if k < n]
    if not ks:
        return empty
    if n != _len0(labels):
        raise ValueError(f"Embeddings and labels must have same length: {n} vs {_len0(labels)}")
    best, best_score = {}, -1.0
    for k, m in _eval(embeds, labels, ks, random_state, silhouette):
        if m["clustering_ari"] > best_score:
            best_score = m["clustering_ari"]
            best = {"clustering_best_k": float(k), "clustering_ari_best": m["clustering_ari"], "clustering_nmi_best": m["clustering_nmi"],
                    "clustering_v_measure_best": m["clustering_v_measure"]}
            if silhouette:
                best["clustering_silhouette_best"] = m["clustering_silhouette"]
    return best if best else empty
