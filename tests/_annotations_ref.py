"""NumPy / plain-Python restatement of avex_amd.annotations: samples, merged reference events, cells, overlaps, compatibility, the
matching walk (with the in-order pair scan the kernels run, and a brute-force maximum matching to hold both against), counts and AP.
Loops over small inputs; nothing here is shared with the package."""
import math

import numpy as np


def to_samples(t, sr):
    return np.floor(np.asarray(t, dtype=np.float64) * float(sr) + 0.5).astype(np.int64)


def merge(intervals):
    """[(lo, hi)] -> the same stretches with overlapping or touching ones joined, sorted."""
    out = []
    for lo, hi in sorted((int(a), int(b)) for a, b in intervals if b > a):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(x) for x in out]


def reference_events(recording, class_id, start_s, end_s, sr, n_rec, n_classes):
    """dict (r, c) -> merged [(lo, hi)]; and the flat table in (r, c, lo) order: rec, cls, lo, hi, seg_offsets, prefix, n_ref."""
    lo, hi = to_samples(start_s, sr), to_samples(end_s, sr)
    segs = {(r, c): [] for r in range(n_rec) for c in range(n_classes)}
    for r, c, a, b in zip(recording, class_id, lo, hi):
        segs[(int(r), int(c))].append((a, b))
    segs = {k: merge(v) for k, v in segs.items()}
    rec, cls, flo, fhi, off = [], [], [], [], [0]
    for r in range(n_rec):
        for c in range(n_classes):
            for a, b in segs[(r, c)]:
                rec.append(r); cls.append(c); flo.append(a); fhi.append(b)
            off.append(len(flo))
    flo, fhi = np.asarray(flo, dtype=np.int64), np.asarray(fhi, dtype=np.int64)
    prefix = np.concatenate([[0], np.cumsum(fhi - flo)]).astype(np.int64)
    n_ref = np.bincount(np.asarray(cls, dtype=np.int64), minlength=n_classes).astype(np.int64)
    return segs, dict(recording=np.asarray(rec, dtype=np.int32), class_id=np.asarray(cls, dtype=np.int32), lo=flo, hi=fhi,
                      seg_offsets=np.asarray(off, dtype=np.int64), prefix=prefix, n_ref=n_ref)


def cells(starts, n_samples, window_len, hop_len):
    """The cells of ONE recording's windows: (lo, hi) lists."""
    shift = (window_len - hop_len) // 2
    edge = [0] + [min(max(int(s) + shift, 0), n_samples) for s in starts[1:]] + [n_samples]
    return edge[:-1], edge[1:]


def covered(lo, hi, events):
    """Samples of [lo, hi) inside the disjoint events."""
    return sum(max(0, min(hi, b) - max(lo, a)) for a, b in events)


def overlap(span_lo, span_hi, win_rec, segs, n_classes):
    """covered() of every window's span with every class of its recording (one event at a time, all windows at once)."""
    span_lo, span_hi, win_rec = np.asarray(span_lo, dtype=np.int64), np.asarray(span_hi, dtype=np.int64), np.asarray(win_rec)
    out = np.zeros((len(span_lo), n_classes), dtype=np.int64)
    for (r, c), events in segs.items():
        mine = win_rec == r
        for a, b in events:
            out[mine, c] += np.maximum(0, np.minimum(span_hi[mine], b) - np.maximum(span_lo[mine], a))
    return out.astype(np.int32)


def compatible(p, r, iou):
    inter = min(p[1], r[1]) - max(p[0], r[0])
    union = max(p[1], r[1]) - min(p[0], r[0])
    return inter > 0 and np.float64(inter) >= np.float64(iou) * np.float64(union)


def walk(preds, refs, iou):
    """The definition: the two-pointer walk.  Returns the pairs (i, j)."""
    i = j = 0
    pairs = []
    while i < len(preds) and j < len(refs):
        if compatible(preds[i], refs[j], iou):
            pairs.append((i, j)); i += 1; j += 1
        elif preds[i][1] <= refs[j][1]:
            i += 1
        else:
            j += 1
    return pairs


def compatible_pairs(preds, refs, iou):
    return [(i, j) for i, p in enumerate(preds) for j, r in enumerate(refs) if compatible(p, r, iou)]


def scan(preds, refs, iou):
    """What the kernels run: the compatible pairs in (i, j) order, a pair taken iff neither of its events is matched yet."""
    pairs, pm, rm = [], set(), set()
    for i, j in compatible_pairs(preds, refs, iou):
        if i not in pm and j not in rm:
            pairs.append((i, j)); pm.add(i); rm.add(j)
    return pairs


def scan_bytes(preds, refs, iou, chunk=4):
    """The same scan as functions on two bits of state composed over chunks, carries and all: the kernels' arithmetic, restated."""
    cp = compatible_pairs(preds, refs, iou)

    def fn(k):
        np_, nr = k == 0 or cp[k][0] != cp[k - 1][0], k == 0 or cp[k][1] != cp[k - 1][1]
        f = []
        for s in range(4):
            t = s & ~((1 if np_ else 0) | (2 if nr else 0))
            f.append(3 if t == 0 else t)
        return f, np_, nr

    def compose(f, g):
        return [g[f[s]] for s in range(4)]

    ident = [0, 1, 2, 3]
    chunks = [list(range(a, min(a + chunk, len(cp)))) for a in range(0, len(cp), chunk)]
    summ = []
    for ch in chunks:
        f = ident
        for k in ch:
            f = compose(f, fn(k)[0])
        summ.append(f)
    state, pairs = 0, []
    for ch, f_all in zip(chunks, summ):
        s = state
        for k in ch:
            f, np_, nr = fn(k)
            if s & ~((1 if np_ else 0) | (2 if nr else 0)) == 0:
                pairs.append(cp[k])
            s = f[s]
        assert s == f_all[state]
        state = s
    return pairs


def max_matching(preds, refs, iou):
    """Kuhn's augmenting paths over the compatibility graph: the cardinality of a maximum matching."""
    adj = {i: [j for j, r in enumerate(refs) if compatible(p, r, iou)] for i, p in enumerate(preds)}
    owner = {}

    def augment(i, seen):
        for j in adj[i]:
            if j in seen:
                continue
            seen.add(j)
            if j not in owner or augment(owner[j], seen):
                owner[j] = i
                return True
        return False

    return sum(1 for i in adj if augment(i, set()))


def match(pred_rows, cell_lo, cell_hi, table, n_classes, iou):
    """pred_rows: [(sequence, class, first, last)] in decode order, filler rows (first < 0) allowed anywhere behind.
    -> match_of_pred [P], match_of_ref [A], spans [(lo, hi)]."""
    P, A = len(pred_rows), len(table["lo"])
    mop, mor = np.full(P, -1, dtype=np.int32), np.full(A, -1, dtype=np.int32)
    spans = [(0, 0)] * P
    by_seg = {}
    for i, (r, c, f, l) in enumerate(pred_rows):
        if f < 0:
            continue
        spans[i] = (int(cell_lo[f]), int(cell_hi[l]))
        by_seg.setdefault((r, c), []).append(i)
    for (r, c), rows in by_seg.items():
        s = r * n_classes + c
        a, b = int(table["seg_offsets"][s]), int(table["seg_offsets"][s + 1])
        refs = [(int(table["lo"][j]), int(table["hi"][j])) for j in range(a, b)]
        for i, j in walk([spans[k] for k in rows], refs, iou):
            mop[rows[i]] = a + j
            mor[a + j] = rows[i]
    return mop, mor, spans


def ratio(num, den):
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, num.astype(np.float64) / np.where(den != 0, den, 1).astype(np.float64), np.nan)


def scores(pred_rows, peaks, mop, table, n_classes):
    cls = np.asarray([c for _, c, f, _ in pred_rows if f >= 0], dtype=np.int64)
    hit = np.asarray([m >= 0 for (_, _, f, _), m in zip(pred_rows, mop) if f >= 0], dtype=bool)
    n_pred = np.bincount(cls, minlength=n_classes).astype(np.int64)
    tp = np.bincount(cls[hit], minlength=n_classes).astype(np.int64)
    n_ref = table["n_ref"]
    out = dict(n_pred=n_pred, n_ref=n_ref, tp=tp, fp=n_pred - tp, fn=n_ref - tp, precision=ratio(tp, n_pred), recall=ratio(tp, n_ref),
               f1=ratio(2 * tp, n_pred + n_ref))
    out.update(micro_precision=ratio(tp.sum(), n_pred.sum()), micro_recall=ratio(tp.sum(), n_ref.sum()), micro_f1=ratio(2 * tp.sum(), n_pred.sum() + n_ref.sum()))
    has = n_ref > 0
    for name, mask in (("precision", has & (n_pred > 0)), ("recall", has), ("f1", has)):
        out["macro_" + name] = math.fsum(out[name][mask]) / mask.sum() if mask.any() else np.nan
    ap = np.full(n_classes, np.nan)
    for c in range(n_classes):
        if n_ref[c] == 0:
            continue
        rows = [i for i, (_, cc, f, _) in enumerate(pred_rows) if f >= 0 and cc == c]
        rows.sort(key=lambda i: (-float(peaks[i]), i))
        terms, seen = [], 0
        for k, i in enumerate(rows, start=1):
            if mop[i] >= 0:
                seen += 1
                terms.append(seen / k)
        ap[c] = math.fsum(terms) / float(n_ref[c])
    out["average_precision"] = ap
    return out


def iou_of(span, ref):
    inter = min(span[1], ref[1]) - max(span[0], ref[0])
    union = max(span[1], ref[1]) - min(span[0], ref[0])
    return np.float64(inter) / np.float64(union)
