"""NumPy restatement of the retrieval metrics (avex/evaluation/retrieval.py), for machines without the reference or scikit-learn.

The ROC-AUC of a binary relevance vector is the Mann-Whitney statistic with ties counted one half:
    U2 = sum over (positive p, negative n) of 2 [s_p > s_n] + [s_p == s_n]          AUC = U2 / (2 P Q)
so no ROC curve is built: the negatives are sorted once and every positive is located in them.  tests/test_retrieval_cpu.py pins this
file to the real reference's outputs (tests/golden/retrieval.npz); the GPU tests then use it on the device's own similarities.
Top-k order: higher similarity first, then lower index.
"""
import numpy as np


def normed(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True).clip(1e-12)


def collapse_one_hot(labels):
    if labels.ndim == 2 and labels.dtype in (np.float32, np.float64, np.int32, np.int64):
        if np.all(labels.sum(axis=1) == 1):
            return labels.argmax(axis=1)
    return labels


def relevance_self(labels):
    """[N, N] bool: item j is relevant to query i (the diagonal included)."""
    labels = np.asarray(labels)
    lab = labels if labels.ndim == 1 else collapse_one_hot(labels)
    if lab.ndim == 1:
        return lab[:, None] == lab[None, :]
    a = (lab != 0).astype(np.int64)
    return (a @ a.T) > 0


def relevance_cross(query_labels, db_labels):
    """[Nq, Ndb] bool, with the reference's corners (retrieval.py:155-196)."""
    ql, dl = np.asarray(query_labels), np.asarray(db_labels)
    if ql.ndim == 1:
        assert dl.ndim == 1
        return ql[:, None] == dl[None, :]
    cq, cd = collapse_one_hot(ql), collapse_one_hot(dl)
    if cq.ndim == 1 and cd.ndim == 1:
        return cq[:, None] == cd[None, :]
    if dl.ndim == 2:
        return ((ql != 0).astype(np.int64) @ (dl != 0).astype(np.int64).T) > 0
    return np.zeros((ql.shape[0], dl.shape[0]), dtype=bool)


def u2_row(scores, rel):
    """(U2, P, Q) of one query: scores and relevance of the ranked items only."""
    pos, neg = scores[rel], np.sort(scores[~rel])
    lo = np.searchsorted(neg, pos, side="left")
    hi = np.searchsorted(neg, pos, side="right")
    return int(lo.sum() + hi.sum()), int(pos.size), int(neg.size)


def stats_from_sim(sim, rel, self_set, k):
    """The per-query integers from a similarity matrix: what avex_amd.retrieval.retrieval_stats returns."""
    nq, nd = sim.shape
    k = min(k, nd - 1 if self_set else nd)
    u2 = np.zeros(nq, dtype=np.int64)
    n_pos, n_neg, hits = (np.zeros(nq, dtype=np.int64) for _ in range(3))
    valid_auc, valid_prec = np.zeros(nq, dtype=bool), np.zeros(nq, dtype=bool)
    topk = np.zeros((nq, k), dtype=np.int64)
    cols = np.arange(nd)
    for i in range(nq):
        keep = cols != i if self_set else np.ones(nd, dtype=bool)
        s, r = sim[i][keep] + 0.0, rel[i][keep]
        u2[i], n_pos[i], n_neg[i] = u2_row(s, r)
        valid_prec[i] = rel[i].sum() > 1 if self_set else n_pos[i] > 0
        valid_auc[i] = valid_prec[i] and n_pos[i] > 0 and n_neg[i] > 0
        order = np.lexsort((cols[keep], -s))[:k]
        topk[i] = cols[keep][order]
        hits[i] = int(rel[i][topk[i]].sum())
    return {"u2": u2, "n_pos": n_pos, "n_neg": n_neg, "valid_auc": valid_auc, "valid_prec": valid_prec, "topk_idx": topk, "hits": hits, "k": k}


def metrics_from_stats(st):
    va, vp = st["valid_auc"], st["valid_prec"]
    auc = st["u2"][va] / (2.0 * st["n_pos"][va] * st["n_neg"][va])
    prec = st["hits"][vp] / float(st["k"]) if st["k"] else np.zeros(0)
    return (float(np.mean(auc)) if auc.size else 0.0), (float(np.mean(prec)) if prec.size else 0.0)


def self_stats(x, labels, k=1):
    n = normed(np.asarray(x))
    return stats_from_sim(np.matmul(n, n.T), relevance_self(labels), True, k)


def cross_stats(q, q_labels, d, d_labels, k=1):
    return stats_from_sim(np.matmul(normed(np.asarray(q)), normed(np.asarray(d)).T), relevance_cross(q_labels, d_labels), False, k)


def load_golden(golden_dir):
    import json
    import os
    z = np.load(os.path.join(golden_dir, "retrieval.npz"))
    return z, json.loads(str(z["meta"]))
