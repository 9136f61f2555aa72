"""Retrieval metrics on the device: mean per-query ROC-AUC and precision@k over a cosine-similarity ranking.

Reference: ``avex/evaluation/retrieval.py`` (called from ``run_evaluate.py:956-961`` on the cached test embeddings).  The eight public
functions keep the reference's names, argument names, defaults, return keys and ``ValueError`` texts; embeddings and labels may be
NumPy arrays or torch tensors, on the host or on the device -- a device tensor is never copied to the host -- and the results are
Python floats.  The arithmetic runs in ``libavexhip.so`` (``csrc/retrieval.hip``); there is no CPU fallback.

What is computed, and where it differs from the reference in the letter:

* Rows are divided by ``max(||row||, 1e-12)``; similarity is the fp32 dot product of the normalised rows (fp32 operands on the fp32
  MFMA).  **Inputs in fp64 (or f16 / bf16) are converted to fp32 on the device and computed in fp32**; the reference computes in the
  dtype it is given.
* A query's ROC-AUC is ``U2 / (2 P Q)`` with ``U2 = sum over (positive, negative) pairs of 2 [s_p > s_n] + [s_p == s_n]``: the
  Mann-Whitney statistic with ties counted one half, which is what ``sklearn.metrics.roc_auc_score`` returns for binary relevance.
  ``U2`` is a 64-bit integer per query, so a run is bit-reproducible; the division and the mean over queries are fp64.
* precision@k for ``k > 1``: the reference uses ``np.argpartition``, whose choice among ties at the k-th place is unspecified.  Here
  the order is **higher similarity first, then lower index** (for ``k == 1`` that is ``argmax``: lowest index on ties, as the
  reference).  ``k`` may be anything, as in the reference, but after clipping to the number of rankable items it must not exceed
  ``MAX_K`` (32): a larger one raises ``ValueError``.
* ``evaluate_precision_cross_set`` with ``k == n_db > 1``: the reference's ``argpartition(-sim, k)`` raises (``kth`` out of bounds);
  here every database item is returned.
* Labels: 1-D (positive = same label), 2-D with every row summing to exactly 1 (collapsed by ``argmax``), or genuine multi-hot
  (positive = at least one shared active class), with the reference's cross-set corners: a one-hot / multi-hot mix is compared as
  multi-hot, and a 1-D database under 2-D multi-hot queries gives all-zero relevance.  1-D query labels against a 2-D database (an
  elementwise broadcast in the reference that ``roc_auc_score`` rejects) raise ``ValueError``.
* NaN or infinite similarities (NaN / inf embeddings) are not ordered against the rank kernel's padding; the result for such a row is
  unspecified.
* At most ``MAX_DB`` (524 288) database items per call; more raise ``ValueError``.

``retrieval_stats`` is the layer below the eight functions: the per-query integers.  Sharding queries over ranks is not built; the
batch loop is the place a ``rows=(lo, hi)`` argument would go.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._metric_inputs import _as_tensor, _device_of, _joint_ids, _len0, _stream

MAX_K = 32                     # avexhip_retrieval_max_k(): the rank kernel's top-k limit
MAX_DB = 1 << 19               # database items per call: a row's relevance bits live in LDS (64 KiB)
_DEFAULT_BATCH = 2048

__all__ = ["evaluate_auc_roc", "evaluate_auc_roc_batched", "evaluate_auc_roc_cross_set", "evaluate_precision", "evaluate_precision_batched",
           "evaluate_precision_cross_set", "eval_retrieval", "eval_retrieval_cross_set", "retrieval_stats", "MAX_K"]


# ------------------------------------------------------------------------------------------------------------------------------
#  Inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _ndim(x) -> int:
    return x.dim() if isinstance(x, torch.Tensor) else np.asarray(x).ndim


def _non_numeric(x) -> bool:
    return not isinstance(x, torch.Tensor) and np.asarray(x).dtype.kind not in "biuf"


def _label_tensors(query_labels, db_labels=None):
    """Torch tensors over the labels where they live.  Labels of a non-numeric NumPy dtype (strings, objects) become dense integer
    codes, ONE coding over both sets so that `==` between a query and a database label survives."""
    if not (_non_numeric(query_labels) or (db_labels is not None and _non_numeric(db_labels))):
        return _as_tensor(query_labels), None if db_labels is None else _as_tensor(db_labels)
    if db_labels is not None and _non_numeric(query_labels) != _non_numeric(db_labels):
        raise ValueError("query and database labels must both be numeric or both be non-numeric")
    q = np.asarray(query_labels)
    d = q[:0] if db_labels is None else np.asarray(db_labels)
    if q.ndim != 1 or d.ndim != 1:
        raise ValueError(f"labels of dtype {q.dtype} must be 1-D")
    codes = torch.from_numpy(np.unique(np.concatenate([q, d]), return_inverse=True)[1].astype(np.int64).reshape(-1))
    return codes[: q.shape[0]], None if db_labels is None else codes[q.shape[0]:]


def _embeddings(x, dev: torch.device) -> torch.Tensor:
    t = _as_tensor(x)
    if t.dim() != 2:
        raise ValueError("embeddings must be 2-D (N, D)")
    return t.to(dev).to(torch.float32).contiguous()


def _collapse_one_hot(lab: torch.Tensor) -> torch.Tensor:
    """retrieval.py:101-121: a 2-D float32 / float64 / int32 / int64 array whose every row sums to exactly 1 becomes class indices."""
    if lab.dim() == 2 and lab.dtype in (torch.float32, torch.float64, torch.int32, torch.int64) and lab.shape[0] > 0:
        if bool((lab.sum(dim=1) == 1).all()):
            return lab.argmax(dim=1)
    return lab


def _pack(lab: torch.Tensor, dev: torch.device) -> torch.Tensor:
    hot = (lab.to(dev) != 0).to(torch.uint8).contiguous()
    n, c = hot.shape
    words = torch.empty((n, (c + 63) // 64), dtype=torch.int64, device=dev)
    if n:
        _capi.check(_capi.lib().avexhip_retrieval_pack_labels(hot.data_ptr(), n, c, words.data_ptr(), _stream()), "retrieval_pack_labels")
    return words


def _relevance(qlab: torch.Tensor, dlab: Optional[torch.Tensor], dev: torch.device):
    """-> ("ids", q_ids, db_ids) or ("words", q_words, db_words); retrieval.py:124-196."""
    if qlab.dim() not in (1, 2) or (dlab is not None and dlab.dim() not in (1, 2)):
        raise ValueError("labels must be 1-D or 2-D")
    if dlab is None:                                   # self-set: _binary_relevance_matrix
        lab = qlab if qlab.dim() == 1 else _collapse_one_hot(qlab)
        if lab.dim() == 1:
            return ("ids",) + _joint_ids(lab, None, dev)
        if lab.shape[1] == 0:
            raise ValueError("multi-hot labels need at least one class")
        w = _pack(lab, dev)
        return "words", w, w
    if qlab.dim() == 1:                                # _binary_relevance_matrix_cross_set
        if dlab.dim() != 1:
            raise ValueError("1-D query labels need 1-D database labels")
        return ("ids",) + _joint_ids(qlab, dlab, dev)
    cq, cd = _collapse_one_hot(qlab), _collapse_one_hot(dlab)
    if cq.dim() == 1 and cd.dim() == 1:
        return ("ids",) + _joint_ids(cq, cd, dev)
    if dlab.dim() == 2:
        if dlab.shape[1] != qlab.shape[1] or qlab.shape[1] == 0:
            raise ValueError("query and database multi-hot labels must have the same number of classes")
        return "words", _pack(qlab, dev), _pack(dlab, dev)
    # 1-D database labels under 2-D multi-hot queries: all-zero relevance (retrieval.py:191-194)
    return ("ids", torch.full((qlab.shape[0],), -1, dtype=torch.int32, device=dev), torch.zeros((dlab.shape[0],), dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------------------------------------
#  The per-query integers
# ------------------------------------------------------------------------------------------------------------------------------
def retrieval_stats(query, query_labels, db=None, db_labels=None, k: int = 1, batch_size: int = _DEFAULT_BATCH, return_sim: bool = False,
                    _timing: Optional[dict] = None) -> Dict[str, object]:
    """Rank every query against the database on the device; ``db=None`` ranks the set against itself (the query's own item removed).

    Returns device tensors, one entry per query: ``u2`` (int64, twice the Mann-Whitney U), ``n_pos`` / ``n_neg`` (ranked items that are /
    are not relevant), ``valid_auc`` / ``valid_prec`` (the reference's skip rules), ``topk_idx`` (``[n_query, k]`` int64, higher
    similarity first, then lower index), ``hits`` (relevant items among them); and the scalars ``k`` (after clipping), ``auc_sum``,
    ``auc_count``, ``prec_sum``, ``prec_count`` (fp64 sums over the valid queries).  ``return_sim=True`` adds ``sim``, the
    ``[n_query, n_db]`` fp32 similarities the ranks were computed from -- for tests, small sets only.  Inputs in fp64 are computed in
    fp32.  Working memory is ``O(batch_size x n_db)``.  ``_timing`` (a dict, for ``scripts/retrieval_bench.py``) launches each batch's
    similarity and rank stages separately, with events between them, and receives ``similarity_s`` / ``rank_s``; the results are the same.
    """
    self_set = db is None
    if self_set and db_labels is not None:
        raise ValueError("db_labels given without db")
    if int(k) < 1:
        raise ValueError("k must be >= 1")
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    if _ndim(query) != 2 or (not self_set and _ndim(db) != 2):
        raise ValueError("embeddings must be 2-D (N, D)")
    n_q = _len0(query)
    n_db = n_q if self_set else _len0(db)
    rankable = n_db - 1 if self_set else n_db
    k_eff = min(int(k), rankable)
    if k_eff > MAX_K:
        raise ValueError(f"k = {k_eff} exceeds the rank kernel's limit of {MAX_K} top items per query")
    if n_db > MAX_DB:
        raise ValueError(f"{n_db} database items exceed the rank kernel's limit of {MAX_DB}")
    _capi.require_gpu()
    dev = _device_of(query, db, query_labels, db_labels)
    with torch.cuda.device(dev):
        if n_q == 0 or rankable <= 0:
            z = torch.zeros((n_q,), dtype=torch.int64, device=dev)
            f = torch.zeros((n_q,), dtype=torch.bool, device=dev)
            out = {"u2": z, "n_pos": z.to(torch.int32), "n_neg": z.to(torch.int32), "valid_auc": f, "valid_prec": f,
                   "topk_idx": torch.zeros((n_q, 0), dtype=torch.int64, device=dev), "hits": z.to(torch.int32), "k": max(k_eff, 0),
                   "auc_sum": 0.0, "auc_count": 0, "prec_sum": 0.0, "prec_count": 0}
            if return_sim:
                out["sim"] = torch.zeros((n_q, max(n_db, 0)), dtype=torch.float32, device=dev)
            return out
        q = _embeddings(query, dev)
        d = q if self_set else _embeddings(db, dev)
        if q.shape[1] != d.shape[1] or q.shape[1] == 0:
            raise ValueError("query and database embeddings must have the same, non-zero width")
        rel = _relevance(*_label_tensors(query_labels, None if self_set else db_labels), dev)
        n_words = 0 if rel[0] == "ids" else int(rel[1].shape[1])
        ql, dl = rel[1], rel[2]
        lib = _capi.lib()
        width = int(q.shape[1])
        batch = min(int(batch_size), n_q)
        ws_bytes = int(lib.avexhip_retrieval_workspace_bytes(n_db, width, batch, n_words))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        u2 = torch.empty((n_q,), dtype=torch.int64, device=dev)
        stats = torch.empty((n_q, 4), dtype=torch.int32, device=dev)
        topk = torch.empty((n_q, MAX_K), dtype=torch.int32, device=dev)
        sim = torch.empty((n_q, n_db), dtype=torch.float32, device=dev) if return_sim else None
        s = _stream()
        _capi.check(lib.avexhip_retrieval_prepare(d.data_ptr(), d.stride(0), n_db, width, batch, ws.data_ptr(), ws_bytes, s), "retrieval_prepare")
        a = _capi.RetrievalArgs()
        a.n_db, a.d, a.batch, a.n_words, a.self_set, a.k, a.stages = n_db, width, batch, n_words, int(self_set), k_eff, 3
        marks = []
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        a.db_ids = dl.data_ptr() if n_words == 0 else None
        a.db_words = dl.data_ptr() if n_words else None
        for b0 in range(0, n_q, batch):
            nb = min(batch, n_q - b0)
            a.nb, a.q0 = nb, b0 if self_set else 0
            a.query, a.ld_query = (None, 0) if self_set else (q.data_ptr() + 4 * b0 * q.stride(0), q.stride(0))
            a.query_ids = ql.data_ptr() + 4 * b0 if n_words == 0 else None
            a.query_words = ql.data_ptr() + 8 * b0 * n_words if n_words else None
            a.u2, a.stats, a.topk = u2.data_ptr() + 8 * b0, stats.data_ptr() + 16 * b0, topk.data_ptr() + 4 * MAX_K * b0
            a.sim_out, a.ld_sim = (sim.data_ptr() + 4 * b0 * n_db, n_db) if return_sim else (None, 0)
            if _timing is None:
                _capi.check(lib.avexhip_retrieval_batch(C.byref(a), s), "retrieval_batch")
                continue
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            for stage in (1, 2):
                a.stages = stage
                _capi.check(lib.avexhip_retrieval_batch(C.byref(a), s), "retrieval_batch")
                ev[stage].record()
            marks.append(ev)
        sums = torch.empty((4,), dtype=torch.float64, device=dev)
        _capi.check(lib.avexhip_retrieval_finalize(u2.data_ptr(), stats.data_ptr(), n_q, int(self_set), k_eff, sums.data_ptr(), s), "retrieval_finalize")
        n_pos, n_neg = stats[:, 0], stats[:, 1]
        valid_prec = (stats[:, 2] > 1) if self_set else (n_pos > 0)
        valid_auc = valid_prec & (n_pos > 0) & (n_neg > 0)
        host = sums.cpu()                                   # the one synchronisation: four doubles
        if _timing is not None:
            _timing["similarity_s"] = sum(e[0].elapsed_time(e[1]) for e in marks) * 1e-3
            _timing["rank_s"] = sum(e[1].elapsed_time(e[2]) for e in marks) * 1e-3
        out = {"u2": u2, "n_pos": n_pos, "n_neg": n_neg, "valid_auc": valid_auc, "valid_prec": valid_prec,
               "topk_idx": topk[:, :k_eff].to(torch.int64), "hits": stats[:, 3], "k": k_eff,
               "auc_sum": float(host[0]), "auc_count": int(host[1]), "prec_sum": float(host[2]), "prec_count": int(host[3])}
        if return_sim:
            out["sim"] = sim
        return out


def _mean(total: float, count: int) -> float:
    return float(total / count) if count else 0.0


def _check_self(embeddings, labels):
    if _ndim(embeddings) != 2:
        raise ValueError("embeddings must be 2-D (N, D)")
    if not isinstance(labels, torch.Tensor):
        labels = np.asarray(labels)
    if _len0(labels) != _len0(embeddings):
        raise ValueError("labels length must match number of embeddings")
    return labels


def _check_cross(query_embeds, query_labels, db_embeds, db_labels):
    if _ndim(query_embeds) != 2 or _ndim(db_embeds) != 2:
        raise ValueError("embeddings must be 2-D (N, D)")
    if not isinstance(query_labels, torch.Tensor):
        query_labels = np.asarray(query_labels)
    if not isinstance(db_labels, torch.Tensor):
        db_labels = np.asarray(db_labels)
    if _len0(query_labels) != _len0(query_embeds):
        raise ValueError("query labels length must match number of query embeddings")
    if _len0(db_labels) != _len0(db_embeds):
        raise ValueError("database labels length must match number of database embeddings")
    return query_labels, db_labels


# ------------------------------------------------------------------------------------------------------------------------------
#  AUC-ROC
# ------------------------------------------------------------------------------------------------------------------------------
def evaluate_auc_roc_batched(embeddings, labels: Sequence[int] | np.ndarray, batch_size: int = 2048) -> float:
    """Mean per-query ROC-AUC of the set ranked against itself (retrieval.py:204-287).

    A query is skipped when its relevance vector, itself included, sums to <= 1, and when no negative is left after its own item is
    removed.  ``batch_size`` queries are ranked per step; the result does not depend on it.  0.0 if no query is valid.
    """
    labels = _check_self(embeddings, labels)
    if _len0(embeddings) <= 1:
        return 0.0
    st = retrieval_stats(embeddings, labels, k=1, batch_size=batch_size)
    return _mean(st["auc_sum"], st["auc_count"])


def evaluate_auc_roc(embeddings, labels: Sequence[int] | np.ndarray) -> float:
    """``evaluate_auc_roc_batched`` with the default batch (retrieval.py:290-354; the full N x N matrix is never formed here)."""
    return evaluate_auc_roc_batched(embeddings, labels)


def evaluate_auc_roc_cross_set(query_embeds, query_labels, db_embeds, db_labels) -> float:
    """Mean per-query ROC-AUC of queries against a separate database (retrieval.py:357-413): nothing is removed; a query with no
    positive or no negative in the database is skipped."""
    query_labels, db_labels = _check_cross(query_embeds, query_labels, db_embeds, db_labels)
    if _len0(query_embeds) == 0 or _len0(db_embeds) == 0:
        return 0.0
    st = retrieval_stats(query_embeds, query_labels, db_embeds, db_labels, k=1)
    return _mean(st["auc_sum"], st["auc_count"])


# ------------------------------------------------------------------------------------------------------------------------------
#  Precision@k
# ------------------------------------------------------------------------------------------------------------------------------
def evaluate_precision_batched(embeddings, labels: Sequence[int] | np.ndarray, k: int = 1, batch_size: int = 2048) -> float:
    """Mean precision@k of the set ranked against itself, the query's own item excluded (retrieval.py:421-510).  ``k`` is clipped to
    ``n - 1``; a query whose relevance vector, itself included, sums to <= 1 is skipped.  Ties: higher similarity first, then lower index."""
    labels = _check_self(embeddings, labels)
    if _len0(embeddings) <= 1:
        return 0.0
    st = retrieval_stats(embeddings, labels, k=k, batch_size=batch_size)
    return _mean(st["prec_sum"], st["prec_count"])


def evaluate_precision(embeddings, labels: Sequence[int] | np.ndarray, k: int = 1) -> float:
    """``evaluate_precision_batched`` with the default batch (retrieval.py:513-585)."""
    return evaluate_precision_batched(embeddings, labels, k=k)


def evaluate_precision_cross_set(query_embeds, query_labels, db_embeds, db_labels, k: int = 1) -> float:
    """Mean precision@k of queries against a separate database (retrieval.py:588-662).  ``k`` is clipped to ``n_db``; a query with no
    positive is skipped, one with no negative counts.  With ``k == n_db > 1`` the reference raises inside ``np.argpartition``; this
    returns every database item instead."""
    query_labels, db_labels = _check_cross(query_embeds, query_labels, db_embeds, db_labels)
    if _len0(db_embeds) == 0 or _len0(query_embeds) == 0:
        return 0.0
    st = retrieval_stats(query_embeds, query_labels, db_embeds, db_labels, k=k)
    return _mean(st["prec_sum"], st["prec_count"])


# ------------------------------------------------------------------------------------------------------------------------------
#  The harness's two calls
# ------------------------------------------------------------------------------------------------------------------------------
def eval_retrieval(embeds, labels, batch_size: int = 2048) -> Dict[str, float]:
    """``{"retrieval_roc_auc", "retrieval_precision_at_1"}`` of a set against itself (retrieval.py:18-46), from one pass."""
    labels = _check_self(embeds, labels)
    if _len0(embeds) <= 1:
        return {"retrieval_roc_auc": 0.0, "retrieval_precision_at_1": 0.0}
    st = retrieval_stats(embeds, labels, k=1, batch_size=batch_size)
    return {"retrieval_roc_auc": _mean(st["auc_sum"], st["auc_count"]), "retrieval_precision_at_1": _mean(st["prec_sum"], st["prec_count"])}


def eval_retrieval_cross_set(query_embeds, query_labels, db_embeds, db_labels) -> Dict[str, float]:
    """The same two metrics for queries against a separate database (retrieval.py:49-91), from one pass."""
    query_labels, db_labels = _check_cross(query_embeds, query_labels, db_embeds, db_labels)
    if _len0(db_embeds) == 0 or _len0(query_embeds) == 0:
        return {"retrieval_roc_auc": 0.0, "retrieval_precision_at_1": 0.0}
    st = retrieval_stats(query_embeds, query_labels, db_embeds, db_labels, k=1)
    return {"retrieval_roc_auc": _mean(st["auc_sum"], st["auc_count"]), "retrieval_precision_at_1": _mean(st["prec_sum"], st["prec_count"])}
