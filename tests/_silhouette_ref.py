"""NumPy restatement of the device silhouette (avex_amd/csrc/silhouette.hip) and the inputs of its golden cases.

The arithmetic restated: rows centred in fp32 ("euclidean": x - fp32(fp64 column mean)) or divided by max(||row||, 1e-12) in fp32
("cosine"); Gram entries G = x.y rounded to fp32; squared norms taken from the DIAGONAL of the same G, so that bit-identical rows
give (||x||^2 + ||y||^2) - 2 x.y == 0 exactly; d = sqrt(max(., 0)) resp. clip(1 - G, 0, 2) in fp32, 0 on the diagonal; per (point,
cluster) sums, a, b, s = (b - a) / max(a, b) and the mean in fp64.  The device rounds after every product of the fp32 MFMA chain, this
file once per Gram entry (an fp64 product rounded to fp32): same form, its own last bits.  tests/test_silhouette_cpu.py pins it to
scikit-learn's float64 result (tests/golden/silhouette.npz) inside the tolerances the device has to meet.

Inputs are regenerated from seeds (CASES); the npz holds expected values only.
"""
import json
import os

import numpy as np

TOL_SAMPLE, TOL_SCORE = 1e-6, 1e-7
METRICS = ("euclidean", "cosine")


def load_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "silhouette.npz"))
    return z, json.loads(str(z["meta"]))


# ------------------------------------------------------------------------------------------------------------------------------
#  Golden inputs
# ------------------------------------------------------------------------------------------------------------------------------
def blobs(seed, n, d, k, sep=1.0, scale=1.0, offset=0.0, sizes=None):
    """rows = scale * (sep * N(0, 1) cluster means + N(0, 1)) + offset, fp32; labels 0 .. k - 1 (random, or blocks of `sizes`, shuffled)."""
    rng = np.random.default_rng(seed)
    if sizes is None:
        lab = rng.integers(0, k, size=n)
        lab[:k] = np.arange(k)                       # every label occurs
    else:
        lab = np.repeat(np.arange(len(sizes)), sizes)
        assert lab.size == n and len(sizes) == k
    means = sep * rng.standard_normal((k, d))
    x = (scale * (means[lab] + rng.standard_normal((n, d))) + offset).astype(np.float32)
    perm = rng.permutation(n)
    return x[perm], lab[perm].astype(np.int64)


def _c300():
    return blobs(11, 300, 40, 5)


def _c515():
    return blobs(12, 515, 37, 7, scale=100.0, offset=50.0)


def _c1000():
    return blobs(13, 1000, 768, 12, sep=0.15)


def _c2000():
    return blobs(14, 2000, 768, 30, sep=1.0)


def _k2():
    return blobs(15, 257, 24, 2)


def _kn1():
    x, _ = blobs(16, 130, 16, 1)
    lab = np.arange(130, dtype=np.int64)
    lab[129] = 0                                     # 129 labels on 130 points: one pair, 128 clusters of one
    return x, lab


def _intlabels():
    x, lab = blobs(17, 200, 20, 3)
    return x, np.array([-3, 7, 1000], dtype=np.int64)[lab]


def _strlabels():
    x, lab = blobs(18, 200, 20, 3)
    return x, np.array(["wren", "finch", "owl"])[lab]


def _singletons():
    x, lab = blobs(19, 150, 12, 4)
    lab = lab.copy()
    lab[[7, 40, 77, 101, 149]] = [4, 5, 6, 7, 8]     # five clusters of one
    return x, lab


def _sizes():
    return blobs(20, 480, 24, 6, sizes=[31, 32, 33, 127, 128, 129])


def _duplicates():
    x, lab = blobs(21, 260, 32, 4)
    x = x.copy()
    rows = np.flatnonzero(lab == 2)
    x[rows] = x[rows[0]]                             # one whole cluster is copies of one row
    return x, lab


CASES = {"c300": _c300, "c515_offset": _c515, "c1000_d768": _c1000, "c2000_d768": _c2000, "k2": _k2, "k_n_minus_1": _kn1, "int_labels": _intlabels,
         "str_labels": _strlabels, "singletons": _singletons, "sizes_31_129": _sizes, "duplicates": _duplicates}
SAMPLED = {"c515_offset": [(200, 0), (200, 7)]}      # case -> (sample_size, random_state)


# ---- past the shapes of silhouette.npz: D > 1024, hundreds of labels.  Expected values in tests/golden/metrics_wide.npz ("sil/<case>/<metric>")
def _w2600():
    return blobs(5, 2600, 1280, 200, sep=0.3)


def _w400():
    return blobs(6, 400, 1536, 6, sep=0.15)


def _many_labels():
    sizes = np.random.default_rng(7).integers(2, 5, size=1000).tolist() + [1] * 5      # 1000 labels of 2 - 4 points, five of one
    return blobs(7, int(np.sum(sizes)), 24, len(sizes), sizes=sizes)


WIDE_CASES = {"w2600_d1280_k200": _w2600, "w400_d1536": _w400, "many_labels_k1005": _many_labels}
MFMA_MARGIN = 14.0      # what the tolerances leave over the emulation's error for the MFMA's summation order (tests/test_gpu_silhouette.py)


def case_inputs(name):
    return (CASES[name] if name in CASES else WIDE_CASES[name])()


def wide_bars(rec, metric):
    """(per-sample bar, score bar) of a record of metrics_wide.npz: the constants where they leave MFMA_MARGIN x the recorded error of this
    file's emulation against scikit-learn float64, MFMA_MARGIN x that error otherwise."""
    es, ec = rec["restatement_max_err"][metric], rec["restatement_score_err"][metric]
    return (TOL_SAMPLE if TOL_SAMPLE >= MFMA_MARGIN * es else MFMA_MARGIN * es), (TOL_SCORE if TOL_SCORE >= MFMA_MARGIN * ec else MFMA_MARGIN * ec)


def sample_indices(n, sample_size, random_state):
    """scikit-learn's subsample: check_random_state(random_state).permutation(n)[:sample_size] (silhouette_score)."""
    return np.random.RandomState(random_state).permutation(n)[:sample_size]


# ------------------------------------------------------------------------------------------------------------------------------
#  The restatement
# ------------------------------------------------------------------------------------------------------------------------------
def rows_for(x, metric):
    x = np.asarray(x, dtype=np.float32)
    if metric == "euclidean":
        mean = (x.sum(axis=0, dtype=np.float64) / x.shape[0]).astype(np.float32)
        return x - mean
    if metric == "cosine":
        nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        return x / np.maximum(nrm, np.float32(1e-12))[:, None]
    raise ValueError(metric)


def distances(x, metric):
    r = rows_for(x, metric)
    r64 = r.astype(np.float64)
    g = (r64 @ r64.T).astype(np.float32)
    g = np.maximum(g, g.T)                           # one value per unordered pair, as x.y == y.x on the device
    if metric == "euclidean":
        inv = np.unique(r, axis=0, return_inverse=True)[1].reshape(-1)
        for u in np.flatnonzero(np.bincount(inv) > 1):      # bit-identical rows: x.y IS the norm (the device takes both from one product)
            rows = np.flatnonzero(inv == u)
            g[np.ix_(rows, rows)] = g[rows[0], rows[0]]
        nr = np.diagonal(g).copy()
        d2 = (nr[:, None] + nr[None, :]) - np.float32(2.0) * g
        d = np.sqrt(np.maximum(d2, np.float32(0.0)))
    else:
        d = np.clip(np.float32(1.0) - g, np.float32(0.0), np.float32(2.0))
    np.fill_diagonal(d, 0.0)
    return d


def silhouette_samples(x, labels, metric="euclidean"):
    ids = np.unique(np.asarray(labels), return_inverse=True)[1].reshape(-1)
    k = int(ids.max()) + 1
    n = ids.shape[0]
    if not 1 < k < n:
        raise ValueError(f"Number of labels is {k}. Valid values are 2 to n_samples - 1 (inclusive)")
    d = distances(x, metric).astype(np.float64)
    onehot = np.zeros((n, k))
    onehot[np.arange(n), ids] = 1.0
    sums = d @ onehot
    counts = onehot.sum(axis=0)
    own = sums[np.arange(n), ids]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = own / (counts[ids] - 1.0)
        other = sums / counts[None, :]
        other[np.arange(n), ids] = np.inf
        b = other.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s[counts[ids] == 1] = 0.0
    return np.nan_to_num(s)


def silhouette_score(x, labels, metric="euclidean", sample_size=None, random_state=None):
    x, labels = np.asarray(x), np.asarray(labels)
    if sample_size is not None:
        idx = sample_indices(x.shape[0], sample_size, random_state)
        x, labels = x[idx], labels[idx]
    s = silhouette_samples(x, labels, metric)
    return float(s.sum() / s.shape[0])
