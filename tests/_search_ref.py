"""NumPy restatement of avex_amd.search: prepared rows, the order of a top-k, greedy temporal suppression, the exclusion masks.

A test module, not a product one: test_search_cpu.py checks it against hand-written cases, test_gpu_search.py compares the device with it.
"""
import numpy as np


def prepared(x, metric="cosine"):
    """Rows as the index keeps them, in fp32: divided by max(||row||, 1e-12) for cosine, as they are for dot.  (The device sums the
    squares in another order; the GPU tests use inputs whose norms are exact, or read the device's own prepared rows.)"""
    x = np.asarray(x, dtype=np.float32)
    if metric == "dot":
        return x.copy()
    if metric != "cosine":
        raise ValueError(metric)
    nrm = np.sqrt((x * x).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return (x / np.maximum(nrm, np.float32(1e-12))[:, None]).astype(np.float32)


def topk_from_sim(sim, k, skip_row=-1, excluded=None):
    """One query's similarities [n] -> (scores [k] fp32, rows [k] int64, count): higher similarity first, then lower row; NaN columns,
    `skip_row` and the columns of the boolean mask `excluded` removed; -inf / -1 past `count`."""
    sim = np.asarray(sim, dtype=np.float32)
    n = sim.shape[0]
    ok = ~np.isnan(sim)
    if excluded is not None:
        ok &= ~np.asarray(excluded, dtype=bool)
    if 0 <= skip_row < n:
        ok[skip_row] = False
    rows = np.flatnonzero(ok)
    s = sim[rows] + np.float32(0.0)                      # -0.0 is ordered, and returned, as +0.0
    order = np.lexsort((rows, -s))                       # the last key is the primary one
    rows, s = rows[order][:k], s[order][:k]
    count = len(rows)
    scores = np.full(k, -np.inf, dtype=np.float32)
    out = np.full(k, -1, dtype=np.int64)
    scores[:count], out[:count] = s, rows
    return scores, out, count


def exclude_mask(mode, q_rec, q_start, q_end, rec, start, end):
    """The database rows one query does not see.  "recording": the rows of its recording (>= 0); "overlap": those of them whose span
    overlaps the query's by a positive amount."""
    rec = np.asarray(rec)
    if mode is None or q_rec < 0:
        return np.zeros(rec.shape[0], dtype=bool)
    same = rec == q_rec
    if mode == "recording":
        return same
    if mode != "overlap":
        raise ValueError(mode)
    start, end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return same & (np.minimum(end, np.float64(q_end)) > np.maximum(start, np.float64(q_start)))


def nms(rows, rec, start, end, max_overlap, k):
    """Greedy suppression over candidate `rows` (best first; global row numbers into rec / start / end): positions, in `rows`, of the
    hits kept.  A candidate falls when a hit already kept has its recording (>= 0) and
    min(end) - max(start) > max_overlap * min(len_a, len_b), in fp64.  Stops at k kept hits."""
    rec = np.asarray(rec)
    start, end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    mo = np.float64(max_overlap)
    kept, kept_rows = [], np.empty(max(k, 1), dtype=np.int64)
    for pos, r in enumerate(rows):
        if len(kept) == k:
            break
        if rec[r] >= 0 and kept:
            o = kept_rows[:len(kept)]
            with np.errstate(invalid="ignore"):
                inter = np.minimum(end[r], end[o]) - np.maximum(start[r], start[o])
                bound = mo * np.minimum(end[r] - start[r], end[o] - start[o])
                if ((rec[o] == rec[r]) & (inter > bound)).any():
                    continue
        kept_rows[len(kept)] = r
        kept.append(pos)
    return kept


def search(sim, k, nms_overlap=None, overfetch=4, skip_rows=None, excluded=None, rec=None, start=None, end=None, max_k=1024):
    """What EmbeddingIndex.search returns, from the similarities [nq, n]: dict of scores, rows, count, recording, start_s, end_s."""
    sim = np.asarray(sim, dtype=np.float32)
    nq, n = sim.shape
    rec = np.full(n, -1, dtype=np.int32) if rec is None else np.asarray(rec, dtype=np.int32)
    start = np.full(n, np.nan) if start is None else np.asarray(start, dtype=np.float64)
    end = np.full(n, np.nan) if end is None else np.asarray(end, dtype=np.float64)
    kp = k if nms_overlap is None else min(k * overfetch, max_k)
    out = {"scores": np.full((nq, k), -np.inf, dtype=np.float32), "rows": np.full((nq, k), -1, dtype=np.int64), "count": np.zeros(nq, dtype=np.int32),
           "recording": np.full((nq, k), -1, dtype=np.int32), "start_s": np.full((nq, k), np.nan), "end_s": np.full((nq, k), np.nan)}
    for q in range(nq):
        s, r, c = topk_from_sim(sim[q], kp, -1 if skip_rows is None else int(skip_rows[q]), None if excluded is None else excluded[q])
        s, r = s[:c], r[:c]
        if nms_overlap is not None:
            keep = nms(r, rec, start, end, nms_overlap, k)
            s, r = s[keep], r[keep]
        c = len(r)
        out["count"][q] = c
        out["scores"][q, :c], out["rows"][q, :c] = s, r
        out["recording"][q, :c], out["start_s"][q, :c], out["end_s"][q, :c] = rec[r], start[r], end[r]
    return out
