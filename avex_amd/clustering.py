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

__all__ = ["eval_clustering", "eval_clustering_multiple_k", "kmeans", "clustering_scores", "MAX_K"]


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


def _reduce_labels(labels) -> torch.Tensor:
    """clustering.py:66-72: [N, 1] squeezed, wider label matrices reduced by argmax."""
    lab = _as_tensor(labels)
    if lab.dim() > 1:
        lab = lab.squeeze() if lab.shape[1] == 1 else lab.argmax(dim=1)
    return lab.reshape(-1)


def _eval_prepared(prep: _Prepared, true_ids: torch.Tensor, n_true: int, k: int, random_state) -> Dict[str, float]:
    dev = prep.x.device
    run = _run(prep, k, 300, random_state, None)
    out = torch.empty((3,), dtype=torch.float64, device=dev)
    _scores_launch(true_ids, n_true, run["labels"], k, out)
    host = torch.cat([out, run["_summary"].to(torch.float64)]).cpu()      # the scores and the finite flag in one read-back
    if not bool(host[3 + 2]):
        logger.error("Clustering evaluation failed: Input X contains NaN or infinity.")
        return _get_empty_clustering_metrics()
    return {"clustering_ari": float(host[0]), "clustering_nmi": float(host[1]), "clustering_v_measure": float(host[2])}


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


def _eval(embeds, labels, ks, random_state):
    """[(k, metrics)] for every k in ks (None = the number of distinct labels >= 0): the data is centred and uploaded once."""
    n = _len0(embeds)
    if _as_tensor(embeds).dim() != 2:
        return [(k, _get_empty_clustering_metrics()) for k in ks]      # scikit-learn raises on anything but a 2-D array: swallowed
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
                res.append((k, _get_empty_clustering_metrics()))
            else:
                res.append((k, _eval_prepared(prep, true_ids, n_true, k, random_state)))
        return res


def eval_clustering_multiple_k(embeds, labels, k_range: Optional[tuple] = None, random_state: int = 42) -> Dict[str, float]:
    """The best of ``eval_clustering`` over a range of k, by ARI, the first on ties (clustering.py:114-190): ``{"clustering_best_k",
    "clustering_ari_best", "clustering_nmi_best", "clustering_v_measure_best"}``.  Default range: ``max(2, true_k - 2) ..
    min(N // 2, true_k + 3)``; the range stops at ``k >= N``.  The data is centred and uploaded once."""
    if _numel(embeds) == 0 or _numel(labels) == 0:
        logger.warning("Empty embeddings or labels provided to clustering evaluation")
        return _get_empty_clustering_best_metrics()
    n = _len0(embeds)
    if k_range is None:
        lab = _reduce_labels(labels)
        true_k = int((torch.unique(lab) >= 0).sum())
        k_range = (max(2, true_k - 2), min(n // 2, true_k + 3))
    ks = [k for k in range(int(k_range[0]), int(k_range[1]) + 1) if k < n]
    if not ks:
        return _get_empty_clustering_best_metrics()
    if n != _len0(labels):
        raise ValueError(f"Embeddings and labels must have same length: {n} vs {_len0(labels)}")
    best, best_score = {}, -1.0
    for k, m in _eval(embeds, labels, ks, random_state):
        if m["clustering_ari"] > best_score:
            best_score = m["clustering_ari"]
            best = {"clustering_best_k": float(k), "clustering_ari_best": m["clustering_ari"], "clustering_nmi_best": m["clustering_nmi"],
                    "clustering_v_measure_best": m["clustering_v_measure"]}
    return best if best else _get_empty_clustering_best_metrics()
