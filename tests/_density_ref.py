"""The semantics of avex_amd.density in dense NumPy (the module docstring of avex_amd/density.py, restated): from rows, or from a given
matrix of similarities (the device's own, so that a test compares decisions and not roundings)."""
import numpy as np

NONE = -1
METRICS = ("cosine", "euclidean")
# the scikit-learn comparison (tests/golden/make_density_goldens.py records it): planted(case_name(n, d), n, d), both metrics
CASES = [(n, d) for n in (129, 257, 300, 384) for d in (5, 33, 48)]
MIN_SAMPLES = 4
MIN_GAP = {"cosine": 3e-5, "euclidean": 4e-4}      # the gap eps sits in must be at least this wide: no pair at the threshold


def case_name(n, d):
    return f"density-planted-{n}-{d}"


def prepared(x, metric):
    """cosine: rows / max(||row||, 1e-12) in fp32; euclidean: rows minus the fp32 column mean (fp64 sum over N, rounded to fp32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if metric not in METRICS:
        raise ValueError(metric)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == "cosine":
            nrm = np.sqrt((x * x).sum(axis=1, dtype=np.float32), dtype=np.float32)
            return (x / np.maximum(nrm, np.float32(1e-12))[:, None]).astype(np.float32)
        mean = (x.astype(np.float64).sum(axis=0) / x.shape[0]).astype(np.float32)
        return (x - mean[None, :]).astype(np.float32)


def similarities(rows, metric):
    p = prepared(rows, metric)
    with np.errstate(invalid="ignore", over="ignore"):
        return (p @ p.T).astype(np.float32)


def distances(sim, metric):
    """fp32 distances from the similarities; the squared norms are their diagonal."""
    s = np.asarray(sim, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == "cosine":
            return np.minimum(np.maximum(np.float32(1.0) - s, np.float32(0.0)), np.float32(2.0))
        nx = np.diagonal(s)
        d2 = (nx[:, None] + nx[None, :]) - np.float32(2.0) * s
        return np.sqrt(np.maximum(d2, np.float32(0.0)), dtype=np.float32)


def dbscan(rows=None, eps=0.5, min_samples=5, metric="cosine", sim=None):
    """labels, core, n_neighbors [N]; sizes, exemplar [n_clusters]; n_clusters, nonfinite."""
    s = similarities(rows, metric) if sim is None else np.asarray(sim, dtype=np.float32)
    n = s.shape[0]
    inside = np.isfinite(np.diagonal(s))
    with np.errstate(invalid="ignore"):
        nb = (distances(s, metric) <= np.float32(eps)) | np.eye(n, dtype=bool)
    nb &= inside[:, None] & inside[None, :]
    assert np.array_equal(nb, nb.T)
    count = nb.sum(axis=1).astype(np.int32)
    core = count >= min_samples
    labels = np.full(n, NONE, dtype=np.int32)
    n_clusters = 0
    for i in range(n):                              # components of the core rows, numbered by their lowest core row
        if not core[i] or labels[i] != NONE:
            continue
        labels[i] = n_clusters
        stack = [i]
        while stack:
            a = stack.pop()
            for b in np.flatnonzero(nb[a] & core & (labels == NONE)):
                labels[b] = n_clusters
                stack.append(int(b))
        n_clusters += 1
    for i in np.flatnonzero(~core):                 # border rows: the smallest number among the core neighbours
        m = nb[i] & core
        if m.any():
            labels[i] = labels[m].min()
    sizes = np.bincount(labels[labels >= 0], minlength=n_clusters).astype(np.int32)
    exemplar = np.full(n_clusters, NONE, dtype=np.int32)
    for c in range(n_clusters):
        members = np.flatnonzero(core & (labels == c))
        exemplar[c] = members[np.argmax(count[members])]      # the first of the largest: the lower row on a tie
    return {"labels": labels, "core": core, "n_neighbors": count, "sizes": sizes, "exemplar": exemplar, "n_clusters": n_clusters,
            "nonfinite": int((~inside).sum())}


def k_distance(sim, k):
    """min(max(1 - s, 0), 2) for the k-th largest similarity of every row to another row; inf where there are fewer than k numbers."""
    s = np.array(sim, dtype=np.float32)
    n = s.shape[0]
    out = np.full(n, np.inf, dtype=np.float32)
    for i in range(n):
        others = np.delete(s[i], i)
        others = np.sort(others[~np.isnan(others)])[::-1]
        if len(others) >= k:
            out[i] = min(max(np.float32(1.0) - others[k - 1], np.float32(0.0)), np.float32(2.0))
    return out


def planted(name, n, d, n_centres=4, sigma=0.4):
    """The planted inputs of the scikit-learn comparison: n_centres Gaussian clusters of width sigma around unit-normal centres (synth names)."""
    from avex_amd import synth
    centres = synth.normal(f"{name}-c", (n_centres, d), 1.0)
    which = np.arange(n) % n_centres
    return (centres[which] + synth.normal(f"{name}-x", (n, d), sigma)).astype(np.float32)


def gap_eps(x, metric, quantile=0.05, places=400):
    """eps = the midpoint of the widest gap among the sorted pairwise fp64 distances within +-places of the quantile; (eps, gap)."""
    x = np.asarray(x, dtype=np.float64)
    if metric == "cosine":
        p = x / np.maximum(np.linalg.norm(x, axis=1), 1e-12)[:, None]
        dist = 1.0 - p @ p.T
    else:
        dist = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))      # direct differences: small inputs only
    v = np.sort(dist[np.triu_indices(x.shape[0], 1)])
    at = int(quantile * len(v))
    lo, hi = max(at - places, 0), min(at + places, len(v) - 1)
    gaps = np.diff(v[lo:hi + 1])
    g = int(np.argmax(gaps))
    return float(0.5 * (v[lo + g] + v[lo + g + 1])), float(gaps[g])
