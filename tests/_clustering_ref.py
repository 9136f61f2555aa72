"""NumPy restatement of the clustering metrics (avex/evaluation/clustering.py), for machines without the reference or scikit-learn.

scikit-learn's seeded KMeans as the device library computes it -- the RandomState protocol, greedy k-means++ seeding, Lloyd's algorithm
with the strict / tolerance stopping rules and the empty-cluster relocation, selection by inertia -- and the three scores from a
contingency table.  tests/test_clustering_cpu.py pins this file to the real reference's outputs (tests/golden/clustering.npz); the GPU
tests then compare the device against it stage by stage.  Written from the algorithm, not from scikit-learn's sources.

Where the order of the arithmetic is free this file follows the device kernels (csrc/clustering.hip), so that most stages agree bit
for bit: seeding distances are direct differences summed over the columns in ascending order in fp32, centre sums add the rows in
ascending order in fp32 (``np.add.at``), centres are ``sum * (1 / count)``.  The assign product is a NumPy GEMM: its last bits differ
from the MFMA's.
"""
import hashlib
import json
import os

import numpy as np

ZERO = {"clustering_ari": 0.0, "clustering_nmi": 0.0, "clustering_v_measure": 0.0}
ZERO_BEST = {"clustering_best_k": 0.0, "clustering_ari_best": 0.0, "clustering_nmi_best": 0.0, "clustering_v_measure_best": 0.0}


def load_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "clustering.npz"))
    return z, json.loads(str(z["meta"]))


def load_wide(golden_dir):
    """tests/golden/metrics_wide.npz (tests/golden/make_metrics_wide_goldens.py): the clustering cases under meta["cases"] and
    "<case>/km_labels", "<case>/seeds0" as in clustering.npz, the silhouette cases under meta["silhouette"] and "sil/<case>/<metric>"."""
    z = np.load(os.path.join(golden_dir, "metrics_wide.npz"))
    return z, json.loads(str(z["meta"]))


def separated(seed, k, per, d, sep=4.0):
    """k well-separated classes of `per` points each, shuffled: rows = sep * N(0, 1) class means + N(0, 1), fp32.  With a few points per
    class and as many centres as classes a point's nearest centre is nearer than the second by a margin, not by luck."""
    rng = np.random.default_rng(seed)
    lab = rng.permutation(np.repeat(np.arange(k), per))
    means = sep * rng.standard_normal((k, d))
    return (means[lab] + rng.standard_normal((k * per, d))).astype(np.float32), lab.astype(np.int64)


def duplicate_init(x, k, copies, seed):
    """[k, D] explicit init: k - copies + 1 distinct rows of x, the first of them `copies` times (at shuffled positions): after the first
    assign copies - 1 clusters are empty, the first copy wins every tie."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(x.shape[0], size=k - copies + 1, replace=False)
    pick = rng.permutation(np.concatenate([np.full(copies, rows[0]), rows[1:]]))
    return x[pick].copy()


SCORES_TABLE = {"seed": 11, "n": 20000, "na": 300, "nb": 350}


def label_pair(seed, n, na, nb):
    """Two label vectors whose contingency table has about na x nb occupied classes: b follows a on 60 % of the points, the rest is uniform."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, na, size=n)
    b = np.where(rng.random(n) < 0.6, (a * 13 + 5) % nb, rng.integers(0, nb, size=n))
    return a.astype(np.int64), b.astype(np.int64)


def assign_margin(x, init, iters, tol=1e-4):
    """The smallest over the first `iters` assigns of Lloyd's algorithm from `init` (the restatement's centres, distances in fp64) and
    over the points of (second nearest - nearest squared distance) / nearest, bit-identical centres counted once; inf where the nearest is 0."""
    xc, mean, _ = prepare(x, tol)
    xnorm = np.einsum("ij,ij->i", xc, xc).astype(np.float32)
    centres = (np.asarray(init, dtype=np.float32) - mean).astype(np.float32)
    worst = np.inf
    for _ in range(iters):
        c64 = np.unique(centres, axis=0).astype(np.float64)
        x64 = xc.astype(np.float64)
        d2 = np.maximum((x64 ** 2).sum(axis=1)[:, None] - 2.0 * x64 @ c64.T + (c64 ** 2).sum(axis=1)[None, :], 0.0)
        d2.sort(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(d2[:, 0] > 0.0, (d2[:, 1] - d2[:, 0]) / d2[:, 0], np.inf)
        worst = min(worst, float(ratio.min()))
        lab, part = assign(xc, centres)
        centres, _ = update(xc, xnorm, centres, lab, part)
    return worst


def clustered(seed, n, d, classes, sep):
    """The generator of the large golden inputs: rows = sep * N(0, 1) class means + unit normal noise, fp32."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, classes, size=n)
    means = sep * rng.standard_normal((classes, d))
    x = (means[lab] + rng.standard_normal((n, d))).astype(np.float32)
    return x, lab.astype(np.int64)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_inputs(z, meta, name):
    """(x fp32, labels) of a golden case: stored, or regenerated from its seed and checked against the recorded SHA-256."""
    c = meta["cases"][name]
    if "gen" in c:
        g = c["gen"]
        x, lab = clustered(g["seed"], g["n"], g["d"], g["classes"], g["sep"])
        assert sha256(x, lab) == c["sha256"], f"{name}: regenerated inputs differ from the ones the golden was made from"
    else:
        x, lab = z[f"{name}/x"], z[f"{name}/labels"]
    return x, lab


# ------------------------------------------------------------------------------------------------------------------------------
#  Random numbers
# ------------------------------------------------------------------------------------------------------------------------------
def trials(k):
    return 2 + int(np.log(k))


def draws(n, k, n_init, random_state):
    """Everything KMeans.fit takes from its RandomState, in stream order: per restart the first centre (a weighted choice over uniform
    fp32 weights) and, for each further centre, 2 + int(ln k) uniforms.  Lloyd's algorithm draws nothing."""
    rs = np.random.RandomState(random_state)
    t = trials(k)
    first = np.zeros(n_init, dtype=np.int64)
    u = np.zeros((n_init, max(k - 1, 0), t), dtype=np.float64)
    w = np.ones(n, dtype=np.float32)
    p = w / w.sum()
    for r in range(n_init):
        first[r] = rs.choice(n, p=p)
        for c in range(k - 1):
            u[r, c] = rs.uniform(size=t)
    return first, u


# ------------------------------------------------------------------------------------------------------------------------------
#  Preparation and seeding
# ------------------------------------------------------------------------------------------------------------------------------
def prepare(x, tol=1e-4):
    x = np.asarray(x, dtype=np.float32)
    mean = (x.sum(axis=0, dtype=np.float64) / x.shape[0]).astype(np.float32)
    xc = x - mean
    var = (xc.astype(np.float64) ** 2).sum(axis=0) / x.shape[0]
    return xc, mean, float(var.mean() * tol)


def sq_dists_seq(xc, rows):
    """[len(rows), N] squared distances, fp32, the columns added one after the other in ascending order (what the seeding kernel does)."""
    c = xc[rows]
    acc = np.zeros((c.shape[0], xc.shape[0]), dtype=np.float32)
    for j in range(xc.shape[1]):
        df = c[:, j][:, None] - xc[:, j][None, :]
        acc = acc + df * df
    return acc


def seed_one(xc, k, first, u):
    n = xc.shape[0]
    chosen = [int(first)]
    closest = sq_dists_seq(xc, [int(first)])[0]
    pot = closest.sum(dtype=np.float64)
    for c in range(1, k):
        cum = np.cumsum(closest.astype(np.float64))
        cand = np.minimum(np.searchsorted(cum, u[c - 1] * pot, side="left"), n - 1)
        dist = np.minimum(closest[None, :], sq_dists_seq(xc, cand))
        pots = dist.sum(axis=1, dtype=np.float64)
        b = int(np.argmin(pots))
        chosen.append(int(cand[b]))
        closest, pot = dist[b], pots[b]
    return np.array(chosen, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
#  Lloyd
# ------------------------------------------------------------------------------------------------------------------------------
def assign(xc, centres):
    cn = np.einsum("ij,ij->i", centres, centres).astype(np.float32)
    part = cn[None, :] - np.float32(2.0) * (xc @ centres.T)
    lab = np.argmin(part, axis=1)
    return lab, part[np.arange(xc.shape[0]), lab]


def update(xc, xnorm, centres, lab, part):
    k = centres.shape[0]
    sums = np.zeros_like(centres)
    np.add.at(sums, lab, xc)                              # rows added in ascending order, fp32
    counts = np.bincount(lab, minlength=k).astype(np.int64)
    empty = np.flatnonzero(counts == 0)
    if empty.size:
        dist = (part + xnorm).astype(np.float32)
        order = np.lexsort((np.arange(dist.size), -dist.astype(np.float64)))      # farthest first, lower index on ties
        for e, p in zip(empty, order[: empty.size]):
            sums[lab[p]] = sums[lab[p]] - xc[p]
            sums[e] = xc[p]
            counts[lab[p]] -= 1
            counts[e] = 1
    new = sums.copy()
    pos = counts > 0
    new[pos] = sums[pos] * (np.float32(1.0) / counts[pos].astype(np.float32))[:, None]
    shift = float(((new - centres).astype(np.float64) ** 2).sum())
    return new, shift


def lloyd(xc, centres, tol_abs, max_iter=300, trace=None, info=None):
    xnorm = np.einsum("ij,ij->i", xc, xc).astype(np.float32)
    centres = centres.astype(np.float32).copy()
    old = np.full(xc.shape[0], -1, dtype=np.int64)
    strict = False
    n_iter = 0
    for it in range(max_iter):
        lab, part = assign(xc, centres)
        if trace is not None:
            trace.append(lab.copy())
        centres, shift = update(xc, xnorm, centres, lab, part)
        n_iter = it + 1
        if np.array_equal(lab, old):
            strict = True
            break
        if shift <= tol_abs:
            break
        old = lab
    if not strict:
        lab, _ = assign(xc, centres)
    if info is not None:
        info["strict"] = strict
    inertia = float(((xc - centres[lab]).astype(np.float32) ** 2).sum(axis=1, dtype=np.float32).astype(np.float64).sum())
    return lab, centres, inertia, n_iter


def kmeans(x, k, n_init=10, max_iter=300, tol=1e-4, random_state=42, init=None, trace=None, info=None):
    """-> dict(labels, centers, inertia, n_iter, best_init, inertias, n_iters, seed_indices), as avex_amd.clustering.kmeans."""
    xc, mean, tol_abs = prepare(x, tol)
    runs, seeds = [], []
    if init is not None:
        runs.append(lloyd(xc, np.asarray(init, dtype=np.float32) - mean, tol_abs, max_iter, trace, info))
    else:
        first, u = draws(xc.shape[0], k, n_init, random_state)
        for r in range(n_init):
            seeds.append(seed_one(xc, k, first[r], u[r]))
            runs.append(lloyd(xc, xc[seeds[-1]], tol_abs, max_iter))
    inertias = np.array([r[2] for r in runs])
    best = int(np.argmin(inertias))                       # the first strictly smallest
    lab, centres, inertia, n_iter = runs[best]
    return {"labels": lab, "centers": centres + mean, "inertia": inertia, "n_iter": n_iter, "best_init": best, "inertias": inertias,
            "n_iters": np.array([r[3] for r in runs]), "seed_indices": np.array(seeds, dtype=np.int64).reshape(len(seeds), k if seeds else 0),
            "all_labels": [r[0] for r in runs]}


# ------------------------------------------------------------------------------------------------------------------------------
#  Scores
# ------------------------------------------------------------------------------------------------------------------------------
def contingency(a, b):
    ia = np.unique(np.asarray(a), return_inverse=True)[1].reshape(-1)
    ib = np.unique(np.asarray(b), return_inverse=True)[1].reshape(-1)
    t = np.zeros((int(ia.max()) + 1, int(ib.max()) + 1), dtype=np.int64)
    np.add.at(t, (ia, ib), 1)
    return t


def scores_from_table(t):
    """(ARI, NMI with the arithmetic mean of the entropies, V-measure with beta = 1) of a contingency table of counts."""
    t = np.asarray(t, dtype=np.int64)
    ra, cb = t.sum(axis=1), t.sum(axis=0)
    ra, cb = ra[ra > 0], cb[cb > 0]
    n = int(t.sum())
    ss = int((t.astype(object) ** 2).sum())
    tp, fp, fn = ss - n, int((cb.astype(object) ** 2).sum()) - ss, int((ra.astype(object) ** 2).sum()) - ss
    tn = n * n - fp - fn - ss
    ari = 1.0 if (fn == 0 and fp == 0) else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))

    def entropy(c):
        if c.size == 1:
            return 0.0
        c = c.astype(np.float64)
        return float(-np.sum((c / n) * (np.log(c) - np.log(n))))

    ha, hb = entropy(ra), entropy(cb)
    mi = 0.0
    if ra.size > 1 and cb.size > 1:
        i, j = np.nonzero(t)
        v = t[i, j].astype(np.float64)
        rows, cols = t.sum(axis=1)[i], t.sum(axis=0)[j]
        nm = v / n
        term = nm * (np.log(v) - np.log(n)) + nm * (-np.log((rows * cols).astype(np.float64)) + np.log(n) + np.log(n))
        term = np.where(np.abs(term) < np.finfo(np.float64).eps, 0.0, term)
        mi = float(max(term.sum(), 0.0))
    if ra.size == 1 and cb.size == 1:
        nmi = 1.0
    elif mi == 0.0:
        nmi = 0.0
    else:
        nmi = mi / (0.5 * (ha + hb))
    hom = mi / ha if ha else 1.0
    com = mi / hb if hb else 1.0
    vm = 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)
    return float(ari), float(nmi), float(vm)


def scores(a, b):
    return scores_from_table(contingency(a, b))


def same_partition(a, b):
    """Two labelings describe the same partition: their contingency table has exactly one non-zero cell per row and per column."""
    t = contingency(a, b)
    return bool(((t > 0).sum(axis=0) == 1).all() and ((t > 0).sum(axis=1) == 1).all())


# ------------------------------------------------------------------------------------------------------------------------------
#  The public functions' rules
# ------------------------------------------------------------------------------------------------------------------------------
def reduce_labels(labels):
    lab = np.asarray(labels)
    if lab.ndim > 1:
        lab = lab.squeeze() if lab.shape[1] == 1 else lab.argmax(axis=1)
    return lab


def eval_clustering(x, labels, n_clusters=None, random_state=42):
    x, raw = np.asarray(x), np.asarray(labels)
    if x.size == 0 or raw.size == 0:
        return dict(ZERO)
    if x.shape[0] != raw.shape[0]:
        raise ValueError(f"Embeddings and labels must have same length: {x.shape[0]} vs {raw.shape[0]}")
    lab = reduce_labels(raw)
    if n_clusters is None:
        uniq = np.unique(lab)
        n_clusters = int((uniq >= 0).sum())
    if n_clusters < 2:
        return dict(ZERO)
    n_clusters = min(n_clusters, x.shape[0])
    if not np.isfinite(x).all():
        return dict(ZERO)
    km = kmeans(x, n_clusters, random_state=random_state)
    ari, nmi, vm = scores(lab, km["labels"])
    return {"clustering_ari": ari, "clustering_nmi": nmi, "clustering_v_measure": vm}
