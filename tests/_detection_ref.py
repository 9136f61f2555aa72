"""NumPy restatement of avex_amd.detection (csrc/events.hip): plain loops, no tricks.

``decode(scores, seq_offsets, on, off, ...)`` takes the ``[N, C]`` score matrix with NaN where a window has no score and returns the
event list in the order (sequence, class_id, first).  Every decision is a compare of fp32 numbers; the fp32 mean of the smoothing adds in
increasing position order and divides by ``float32(n)``, which NumPy's float32 scalars do with the device's bits.
"""
import math

import numpy as np

FIELDS = ("sequence", "class_id", "first", "last", "peak", "peak_window", "mean")


def smooth_sequence(x, smooth, mode):
    """x: the fp32 scores of ONE sequence and class (NaN = no score) -> the smoothed fp32 scores."""
    x = np.asarray(x, dtype=np.float32)
    n, h = len(x), (smooth - 1) // 2
    out = np.empty(n, dtype=np.float32)
    if smooth == 1:
        return x.copy()
    for i in range(n):
        w = x[max(i - h, 0):min(i + h, n - 1) + 1]
        vals = w[~np.isnan(w)]
        if len(vals) == 0:
            out[i] = np.nan
        elif mode == "median":
            out[i] = np.sort(vals)[(len(vals) - 1) // 2]
        elif mode == "mean":
            s = np.float32(0.0)
            for v in vals:
                s = np.float32(s + v)
            out[i] = np.float32(s / np.float32(len(vals)))
        else:
            raise ValueError(mode)
    return out


def hysteresis(s, on, off):
    """Smoothed scores of one sequence and class -> the active flags, starting inactive."""
    on, off = np.float32(on), np.float32(off)
    active, state = [], False
    for v in s:
        if v >= on:
            state = True
        elif not (v >= off):
            state = False
        active.append(state)
    return active


def runs_of(active):
    """[(first, last)] of the maximal runs of True."""
    runs, i, n = [], 0, len(active)
    while i < n:
        if active[i]:
            j = i
            while j + 1 < n and active[j + 1]:
                j += 1
            runs.append((i, j))
            i = j + 1
        else:
            i += 1
    return runs


def merge_runs(runs, merge_gap):
    """An inactive run of at most merge_gap windows strictly between two runs joins them (0 merges nothing)."""
    out = []
    for a, b in runs:
        if out and merge_gap > 0 and a - out[-1][1] - 1 <= merge_gap:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def decode(scores, seq_offsets, on, off=None, smooth=1, smooth_mode="median", merge_gap=0, min_windows=1, stats=None):
    """-> dict of NumPy columns (FIELDS) in the order (sequence, class_id, first).  ``stats`` (a dict) receives the numbers of raw, merged
    and kept runs, and ``mean_terms``: per event the smoothed scores its mean is taken over."""
    scores = np.asarray(scores, dtype=np.float32)
    n, c_all = scores.shape
    on = np.broadcast_to(np.asarray(on, dtype=np.float32), (c_all,))
    off = on if off is None else np.broadcast_to(np.asarray(off, dtype=np.float32), (c_all,))
    ev = {k: [] for k in FIELDS}
    terms = []
    n_raw = n_merged = n_kept = 0
    for r in range(len(seq_offsets) - 1):
        lo, hi = int(seq_offsets[r]), int(seq_offsets[r + 1])
        for c in range(c_all):
            s = smooth_sequence(scores[lo:hi, c], smooth, smooth_mode)
            raw = runs_of(hysteresis(s, on[c], off[c]))
            merged = merge_runs(raw, merge_gap)
            kept = [(a, b) for a, b in merged if b - a + 1 >= min_windows]
            n_raw, n_merged, n_kept = n_raw + len(raw), n_merged + len(merged), n_kept + len(kept)
            for a, b in kept:
                seg = s[a:b + 1]
                good = ~np.isnan(seg)
                peak = seg[good].max()
                ev["sequence"].append(r)
                ev["class_id"].append(c)
                ev["first"].append(lo + a)
                ev["last"].append(lo + b)
                ev["peak"].append(peak)
                ev["peak_window"].append(lo + a + int(np.flatnonzero(good & (seg == peak))[0]))
                vals = [float(v) for v in seg[good]]
                ev["mean"].append(math.fsum(vals) / len(vals))
                terms.append(vals)
    if stats is not None:
        stats.update(raw=n_raw, merged=n_merged, kept=n_kept, mean_terms=terms)
    dt = {"peak": np.float32, "mean": np.float64}
    return {k: np.asarray(v, dtype=dt.get(k, np.int32)) for k, v in ev.items()}


def mean_bound(vals):
    """The first-order bound of an fp64 sum of n terms in any order, plus the division's rounding: n * 2^-52 * (sum |x| / n)."""
    n = len(vals)
    return n * 2.0 ** -52 * (math.fsum(abs(v) for v in vals) / n)
