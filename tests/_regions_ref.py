"""NumPy restatement of avex_amd.regions for the tests: the threshold, the cell mask from a power array, and the connected regions.

Written from the description, not from the package's code: a sequential union-find with explicit loops over a bool mask where the package
packs bits, counts prefixes and hooks with atomics.  Frames, the window and the float64 transform are those of tests/_activity_ref.py.

  threshold   thr[r, k] = maximum(float32(noise[r, k]) * float32(10^(snr_db / 10)), float32(16384 * 10^(min_db / 10))) in float32, the
              maximum keeping a NaN; min_db None: the floor is 0; noise None: the floor alone
  cells       mask[f, k] = lo <= k < hi and P[f, k] > thr[k] (strict; false for a NaN on either side)
  neighbours  two set cells of one recording with |df| <= rt and |dk| <= rk; regions = the connected components; a region's number is
              the rank of its smallest cell by (recording, frame, bin)
  columns     recording, first_frame, last_frame (inside the recording, inclusive), low_bin, high_bin (inclusive), n_cells,
              n_frames = last_frame - first_frame + 1, n_bins = high_bin - low_bin + 1
  filters     min_cells, min_frames, min_bins, max_frames (None: no bound): a region failing one is dropped, the others keep their order
"""
import numpy as np

N_BINS = 257
P_FS = 16384.0
COLUMNS = ("recording", "first_frame", "last_frame", "low_bin", "high_bin", "n_cells", "n_frames", "n_bins")


def ratio32(snr_db):
    return np.float32(10.0 ** (snr_db / 10.0))


def floor32(min_db):
    return np.float32(0.0) if min_db is None else np.float32(np.float64(P_FS) * np.float64(10.0) ** (np.float64(min_db) / 10.0))


def threshold(noise, snr_db, min_db, n_rec):
    """[n_rec, 257] float32.  noise: [n_rec, 257] or None."""
    floor = np.full((n_rec, N_BINS), floor32(min_db), dtype=np.float32)
    if noise is None:
        assert min_db is not None
        return floor
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum(np.asarray(noise, dtype=np.float32) * ratio32(snr_db), floor)      # np.maximum keeps a NaN, like torch.maximum


def mask_of_power(P, thr_row, lo=0, hi=N_BINS):
    """P: [F, 257] of any float dtype (NaN rows for non-finite frames), thr_row: [257] -> bool [F, 257]."""
    with np.errstate(invalid="ignore"):
        m = P > np.asarray(thr_row).astype(P.dtype)[None, :]
    m[:, :lo] = False
    m[:, hi:] = False
    return m


def unpack(cells):
    """The device's [F, 9] int32 words -> bool [F, 257]; asserts that the spare bits of word 8 are clear."""
    w = np.ascontiguousarray(cells).view(np.uint32).astype(np.uint64)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    flat = bits.reshape(len(w), 9 * 32).astype(bool)
    assert not flat[:, N_BINS:].any()
    return flat[:, :N_BINS]


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def label(mask, frames_per_recording, reach=(1, 1), min_cells=1, min_frames=1, min_bins=1, max_frames=None):
    """-> (columns: a dict of int32 arrays over the kept regions, n_found, labels: int32 [F, 257] with the number of each set cell's
    region before the filters, 1-based, 0 elsewhere)."""
    mask = np.asarray(mask, dtype=bool)
    rt, rk = reach
    F = mask.shape[0]
    assert mask.shape == (F, N_BINS) and sum(frames_per_recording) == F
    rec_of, first_of, end_of = np.zeros(F, np.int64), np.zeros(F, np.int64), np.zeros(F, np.int64)
    f = 0
    for r, n in enumerate(frames_per_recording):
        rec_of[f:f + n], first_of[f:f + n], end_of[f:f + n] = r, f, f + n
        f += n
    number = -np.ones((F, N_BINS), dtype=np.int64)           # cells in (recording, frame, bin) order
    cells = [(int(a), int(b)) for a, b in zip(*np.nonzero(mask))]
    for i, (a, b) in enumerate(cells):
        number[a, b] = i
    parent = list(range(len(cells)))
    for i, (a, b) in enumerate(cells):
        for df in range(0, rt + 1):                          # the forward half-neighbourhood
            g = a + df
            if g >= end_of[a]:
                break
            for dk in (range(1, rk + 1) if df == 0 else range(-rk, rk + 1)):
                k = b + dk
                if 0 <= k < N_BINS and mask[g, k]:
                    x, y = _find(parent, i), _find(parent, int(number[g, k]))
                    if x != y:
                        parent[max(x, y)] = min(x, y)
    roots = [_find(parent, i) for i in range(len(cells))]
    order = {}                                               # root -> region number, in the order of the roots (a root is its tree's smallest cell)
    for i, r in enumerate(roots):
        assert r <= i
        if r == i:
            order[r] = len(order)
    n_found = len(order)
    labels = np.zeros((F, N_BINS), dtype=np.int32)
    rows = [dict(recording=None, first_frame=None, last_frame=-1, low_bin=N_BINS, high_bin=-1, n_cells=0) for _ in range(n_found)]
    for i, (a, b) in enumerate(cells):
        g = order[roots[i]]
        labels[a, b] = g + 1
        row, fl = rows[g], a - int(first_of[a])
        if row["recording"] is None:
            row["recording"], row["first_frame"] = int(rec_of[a]), fl
        assert row["recording"] == rec_of[a]
        row["first_frame"], row["last_frame"] = min(row["first_frame"], fl), max(row["last_frame"], fl)
        row["low_bin"], row["high_bin"] = min(row["low_bin"], b), max(row["high_bin"], b)
        row["n_cells"] += 1
    kept = []
    for row in rows:
        row["n_frames"], row["n_bins"] = row["last_frame"] - row["first_frame"] + 1, row["high_bin"] - row["low_bin"] + 1
        if row["n_cells"] >= min_cells and row["n_frames"] >= min_frames and row["n_bins"] >= min_bins and (max_frames is None or row["n_frames"] <= max_frames):
            kept.append(row)
    return {c: np.asarray([row[c] for row in kept], dtype=np.int32) for c in COLUMNS}, n_found, labels


def derived(cols, hop, sr):
    """The float64 columns of the kept regions."""
    first, last = cols["first_frame"].astype(np.int64), cols["last_frame"].astype(np.int64)
    out = {"begin_s": (first * hop).astype(np.float64) / sr, "end_s": (last * hop + 512).astype(np.float64) / sr,
           "low_hz": cols["low_bin"].astype(np.float64) * sr / 512, "high_hz": cols["high_bin"].astype(np.float64) * sr / 512}
    out["bandwidth_hz"] = out["high_hz"] - out["low_hz"] + sr / 512
    out["duration_s"] = out["end_s"] - out["begin_s"]
    return out


def boxes(cols, hop):
    """(recording, start_sample, end_sample, bins [E, 2]) of the kept regions."""
    first, last = cols["first_frame"].astype(np.int64), cols["last_frame"].astype(np.int64)
    return (cols["recording"].astype(np.int64), first * hop, last * hop + 512,
            np.stack([cols["low_bin"].astype(np.int64), cols["high_bin"].astype(np.int64) + 1], axis=1).reshape(-1, 2))
