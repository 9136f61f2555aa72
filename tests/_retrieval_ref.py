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


def stats_from_sim(sim, rel, self_set, k, row0=0):
    """The per-query integers from a similarity matrix: what avex_amd.retrieval.retrieval_stats returns.  `row0`: the rows are queries
    row0 .. row0 + nq - 1 of a self-set (the column a row leaves out is row0 + its index)."""
    nq, nd = sim.shape
    k = min(k, nd - 1 if self_set else nd)
    u2 = np.zeros(nq, dtype=np.int64)
    n_pos, n_neg, hits = (np.zeros(nq, dtype=np.int64) for _ in range(3))
    valid_auc, valid_prec = np.zeros(nq, dtype=bool), np.zeros(nq, dtype=bool)
    topk = np.zeros((nq, k), dtype=np.int64)
    cols = np.arange(nd)
    for i in range(nq):
        keep = cols != row0 + i if self_set else np.ones(nd, dtype=bool)
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


def chunked_case(n0=None, n_db=40001, d=40, per_class=10, seed=7):
    """Cross-set inputs that drive the rank kernel through several sorted chunks (more than 16 384 keys on the smaller side of a query):
    a database of n_db rows made of n_db // 4 distinct rows, each four times at shuffled positions (equal similarities in different
    chunks) plus one more distinct row; class 0 on n0 rows (None: 48 %), class 2 on 30 rows, class 1 on the rest, class 3 on none; the
    labels do not depend on the rows, so copies of a row sit on both sides of a query.  per_class queries of each of the classes 0 .. 3.
    -> q [4 per_class, d] fp32, q_ids, db [n_db, d] fp32, db_ids (int64)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n_db // 4 + 1, d)).astype(np.float32)
    src = np.concatenate([np.repeat(np.arange(n_db // 4), 4), np.arange(n_db // 4, n_db // 4 + n_db % 4 + (n_db % 4 == 0))])[:n_db]
    db = base[rng.permutation(src)]
    n0 = int(round(0.48 * n_db)) if n0 is None else n0
    ids = np.ones(n_db, dtype=np.int64)
    where = rng.permutation(n_db)
    ids[where[:n0]] = 0
    ids[where[n0:n0 + 30]] = 2
    q_ids = np.repeat(np.arange(4, dtype=np.int64), per_class)
    centre = 0.5 * rng.standard_normal((4, d))                                # queries lean towards nothing in the database in particular
    q = (centre[q_ids] + rng.standard_normal((q_ids.size, d))).astype(np.float32)
    q[::3] = db[rng.integers(0, n_db, size=q[::3].shape[0])]                  # every third query IS a database row: similarity 1 with its four copies
    return q, q_ids, db, ids


def multihot_of(ids, extra_col, n_classes=70, columns=(0, 1, 65, 66)):
    """Genuine multi-hot labels (two 64-bit words) with the relevance of the class ids: class c is column columns[c], and every fifth row
    also carries `extra_col` -- give the queries one and the database another, so that it only keeps either matrix from being one-hot."""
    m = np.zeros((ids.shape[0], n_classes), dtype=np.int64)
    m[np.arange(ids.shape[0]), np.asarray(columns)[ids]] = 1
    m[::5, extra_col] = 1
    return m


def load_golden(golden_dir):
    import json
    import os
    z = np.load(os.path.join(golden_dir, "retrieval.npz"))
    return z, json.loads(str(z["meta"]))
