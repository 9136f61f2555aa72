"""NumPy restatement of avex_amd.examples: the per-class value, the two modes, nearest, the prototypes.

A test module, not a product one: test_examples_cpu.py checks it against hand-written cases, test_gpu_examples.py compares the device with it.
Prepared rows are those of _search_ref.prepared.
"""
import numpy as np

MAX_TOP_M = 16


def class_value(sims, top_m):
    """One window's similarities to the rows of one class, in the order the rows were added -> (value fp32, position of the nearest or -1).
    NaN is not counted, -0.0 is +0.0; the min(top_m, count) largest are added in fp32 in descending order from the largest and divided by
    float(count kept); none: NaN.  On equal similarity the earlier row is the nearest."""
    assert 1 <= top_m <= MAX_TOP_M
    s = np.asarray(sims, dtype=np.float32).reshape(-1) + np.float32(0.0)
    pos = np.flatnonzero(~np.isnan(s))
    if pos.size == 0:
        return np.float32(np.nan), -1
    order = pos[np.lexsort((pos, -s[pos]))]                # higher similarity first, then the earlier row
    kept = s[order[:top_m]]
    acc = kept[0]
    for v in kept[1:]:
        acc = np.float32(acc + v)
    with np.errstate(invalid="ignore"):
        return np.float32(acc / np.float32(len(kept))), int(order[0])


def _values(sim, cols, top_m):
    """class_value for every row of sim [N, M] over the columns `cols` (ascending): (values [N] fp32, nearest column [N] or -1)."""
    n = sim.shape[0]
    if len(cols) == 0:
        return np.full(n, np.nan, dtype=np.float32), np.full(n, -1, dtype=np.int64)
    s = sim[:, cols] + np.float32(0.0)
    order = np.argsort(-s, axis=1, kind="stable")          # descending; NaN last; equal values keep the column order
    top = np.take_along_axis(s, order[:, :top_m], axis=1)
    cnt = np.minimum((~np.isnan(s)).sum(axis=1), top_m)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = top[:, 0].copy()
        for i in range(1, top.shape[1]):
            acc = np.where(i < cnt, (acc + top[:, i]).astype(np.float32), acc)
        val = np.where(cnt > 0, (acc / cnt.astype(np.float32)).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    near = np.where(cnt > 0, np.asarray(cols)[order[:, 0]], -1)
    return val, near


def score(sim, labels, n_classes, top_m=1, mode="similarity"):
    """What ExampleBank.score returns, from the similarities [N, M] of the windows to the bank rows in the order they were added and the
    rows' labels (-1: background): (scores [N, C] fp32, nearest [N, C] int32)."""
    sim = np.asarray(sim, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    n = sim.shape[0]
    scores = np.empty((n, n_classes), dtype=np.float32)
    nearest = np.empty((n, n_classes), dtype=np.int32)
    for c in range(n_classes):
        scores[:, c], nearest[:, c] = _values(sim, np.flatnonzero(labels == c), top_m)
    if mode == "margin":
        bg, _ = _values(sim, np.flatnonzero(labels == -1), top_m)
        with np.errstate(invalid="ignore"):
            scores = (scores - bg[:, None]).astype(np.float32)
    elif mode != "similarity":
        raise ValueError(mode)
    return scores, nearest


def prototypes(rows, labels, n_classes):
    """(means [K, d] fp32, labels [K]): per non-empty class, then the background if any, the sum of its prepared rows in the order they
    were added -- sequential fp32 additions from 0, one accumulator per column -- over float(count)."""
    rows = np.asarray(rows, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    out, lab = [], []
    for c in list(range(n_classes)) + [-1]:
        idx = np.flatnonzero(labels == c)
        if idx.size == 0:
            continue
        acc = np.zeros(rows.shape[1], dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in idx:
                acc = (acc + rows[r]).astype(np.float32)
            out.append((acc / np.float32(idx.size)).astype(np.float32))
        lab.append(c)
    return (np.stack(out) if out else np.zeros((0, rows.shape[1]), dtype=np.float32)), np.asarray(lab, dtype=np.int64)
