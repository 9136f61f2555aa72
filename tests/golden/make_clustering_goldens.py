"""Golden generator for avex_amd.clustering: runs the REAL reference (avex/evaluation/clustering.py, imported by the recipe of
tests/golden/_ref_import.py; it needs numpy / torch / scikit-learn) and writes tests/golden/clustering.npz.

Run in the development container only (the reference checkout is not on the GPU box); nothing under tests/ imports this module.
The npz holds data only.  Per case: the reference's result dict; from scikit-learn's KMeans called with the reference's arguments the
winning labels, inertia and n_iter; from sklearn.cluster.kmeans_plusplus with a RandomState the first restart's seed rows.  Large inputs
are regenerated in the tests from a seed (tests/_clustering_ref.clustered) and pinned by the SHA-256 of their bytes; small ones are stored.

Conditions a case must meet to be written (meta["max_unstable"] = 0; a case that fails gets another data seed):
  * the reference's partition does not change when every input is multiplied by 1 + 1e-6 N(0, 1), under three noise seeds;
  * no restart with a DIFFERENT partition comes within MIN_GAP (relative) of the winner's inertia, by the per-restart inertias of the
    NumPy restatement (tests/_clustering_ref.py): a device that sums inertia in another order cannot pick another winner.
"""
import importlib
import json
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _clustering_ref as CR  # noqa: E402

NOISE, NOISE_SEEDS, MIN_GAP = 1e-6, (1, 2, 3), 1e-5


def load_reference():
    sys.path.insert(0, HERE)
    import _ref_import
    _ref_import.import_reference()
    return importlib.import_module("avex.evaluation.clustering")


def ref_kmeans(x, k, random_state=42, **kw):
    from sklearn.cluster import KMeans
    km = KMeans(n_clusters=k, random_state=random_state, n_init=kw.pop("n_init", 10), max_iter=kw.pop("max_iter", 300), **kw)
    lab = km.fit_predict(x)
    return lab.astype(np.int64), float(km.inertia_), int(km.n_iter_)


def ref_seeds(x, k, random_state=42):
    from sklearn.cluster import kmeans_plusplus
    x = np.asarray(x, dtype=np.float32)
    xc = x - x.mean(axis=0)                     # KMeans.fit seeds on the centred data
    return kmeans_plusplus(xc, k, random_state=np.random.RandomState(random_state))[1].astype(np.int64)


def noisy(x, seed):
    return (x.astype(np.float64) * (1.0 + NOISE * np.random.default_rng(seed).standard_normal(x.shape))).astype(np.float32)


def eval_case(R, x, labels, n_clusters=None, gen=None, store_x=True):
    """-> (arrays, meta) or None when a condition fails."""
    import torch
    arrays, m = {}, {}
    ref = R.eval_clustering(torch.from_numpy(x), torch.from_numpy(labels), n_clusters=n_clusters)
    m["eval_clustering"] = ref
    m["n_clusters"] = n_clusters
    lab1 = CR.reduce_labels(labels)
    k = n_clusters if n_clusters is not None else int((np.unique(lab1) >= 0).sum())
    k = min(k, x.shape[0])
    m["k"] = k
    if gen is not None:
        m["gen"], m["sha256"] = gen, CR.sha256(x, labels)
    if store_x:
        arrays["x"] = x
    arrays["labels"] = labels
    if k >= 2 and np.isfinite(x).all():
        lab, inertia, n_iter = ref_kmeans(x, k)
        sc = CR.scores(lab1, lab)
        assert max(abs(sc[0] - ref["clustering_ari"]), abs(sc[1] - ref["clustering_nmi"]), abs(sc[2] - ref["clustering_v_measure"])) <= 1e-12
        arrays["km_labels"] = lab.astype(np.int16)
        arrays["seeds0"] = ref_seeds(x, k)
        m["inertia"], m["n_iter"] = inertia, n_iter
        for s in NOISE_SEEDS:
            if not CR.same_partition(ref_kmeans(noisy(x, s), k)[0], lab):
                print("   unstable under input noise, seed", s)
                return None
        mine = CR.kmeans(x, k)
        same = [CR.same_partition(l, mine["labels"]) for l in mine["all_labels"]]
        win = mine["inertia"]
        gaps = [abs(i - win) / win for i, sm in zip(mine["inertias"], same) if not sm]
        m["restatement_inertias"] = [float(i) for i in mine["inertias"]]
        m["restatement_best_init"] = mine["best_init"]
        m["restarts_with_winning_partition"] = int(sum(same))
        m["nearest_other_partition_gap"] = float(min(gaps)) if gaps else None
        if gaps and min(gaps) < MIN_GAP:
            print("   another partition within", min(gaps), "of the winner's inertia")
            return None
        if not CR.same_partition(mine["labels"], lab):
            print("   NOTE: restatement partition differs from the reference's")
    else:
        assert ref == CR.ZERO
    return arrays, m


def small_set(seed, n, d, classes, sep):
    x, lab = CR.clustered(seed, n, d, classes, sep)
    return x.astype(np.float16).astype(np.float32), lab


def main():
    import torch
    warnings.filterwarnings("ignore")
    R = load_reference()
    out, meta = {}, {"sklearn": __import__("sklearn").__version__, "noise": NOISE, "noise_seeds": list(NOISE_SEEDS), "min_gap": MIN_GAP,
                     "max_unstable": 0, "cases": {}}

    def add(name, build):
        seed = 1000
        while True:
            print(name, "seed", seed, flush=True)
            got = build(seed)
            if got is not None:
                break
            seed += 1
        arrays, m = got
        for key, a in arrays.items():
            out[f"{name}/{key}"] = a
        meta["cases"][name] = m

    def big(n, d, classes, sep, n_clusters=None):
        def build(seed):
            x, lab = CR.clustered(seed, n, d, classes, sep)
            got = eval_case(R, x, lab, n_clusters, gen={"seed": seed, "n": n, "d": d, "classes": classes, "sep": sep}, store_x=False)
            if got is not None:
                got[0].pop("labels")
            return got
        return build

    add("set8", big(2000, 64, 8, 1.0))
    add("set12", big(3000, 128, 12, 0.25))
    add("set20_d768", big(4000, 768, 20, 0.08))
    add("set30_d100", big(1500, 100, 30, 0.3))
    add("set12_k5", big(3000, 128, 12, 0.25, n_clusters=5))
    add("set12_k30", big(3000, 128, 12, 0.25, n_clusters=30))

    def col_labels(seed):
        x, lab = small_set(seed, 301, 24, 5, 1.2)
        return eval_case(R, x, lab.reshape(-1, 1))
    add("labels_n1", col_labels)

    def multihot(seed):
        x, lab = small_set(seed, 260, 20, 6, 1.2)
        rng = np.random.default_rng(seed + 1)
        mh = np.eye(6, dtype=np.int64)[lab]
        extra = rng.integers(0, 6, size=lab.size)
        mh[np.arange(lab.size)[::3], extra[::3]] = 1           # a second active class on every third row: argmax takes the first
        return eval_case(R, x, mh)
    add("multihot", multihot)

    def minus_one(seed):
        x, lab = small_set(seed, 280, 20, 5, 1.2)
        lab = lab.copy()
        lab[::17] = -1                                         # not counted for n_clusters, but a class of its own in the scores
        return eval_case(R, x, lab)
    add("label_minus1", minus_one)

    def n6(seed):
        x, _ = small_set(seed, 6, 10, 3, 1.0)
        return eval_case(R, x, np.array([0, 3, 9, 3, 7, 0], dtype=np.int64), n_clusters=10)      # k clipped to N
    add("n6_k10", n6)

    def one_class(seed):
        x, lab = small_set(seed, 50, 8, 3, 1.0)
        return eval_case(R, x, np.zeros_like(lab))
    add("one_class", one_class)

    def nan_row(seed):
        x, lab = small_set(seed, 90, 12, 3, 1.0)
        x = x.copy()
        x[17, 3] = np.nan
        return eval_case(R, x, lab)
    add("nan_row", nan_row)

    # eval_clustering_multiple_k on the 8-class set
    g = meta["cases"]["set8"]["gen"]
    x, lab = CR.clustered(g["seed"], g["n"], g["d"], g["classes"], g["sep"])
    mk = R.eval_clustering_multiple_k(torch.from_numpy(x), torch.from_numpy(lab))
    for s in NOISE_SEEDS:
        other = R.eval_clustering_multiple_k(torch.from_numpy(noisy(x, s)), torch.from_numpy(lab))
        assert all(abs(other[key] - mk[key]) <= 1e-12 for key in mk), "multiple_k unstable under input noise"
    per_k = {}
    for k in range(6, 12):
        mine = CR.kmeans(x, k)
        same = [CR.same_partition(l, mine["labels"]) for l in mine["all_labels"]]
        gaps = [abs(i - mine["inertia"]) / mine["inertia"] for i, sm in zip(mine["inertias"], same) if not sm]
        assert not gaps or min(gaps) >= MIN_GAP, ("multiple_k", k, min(gaps))
        per_k[str(k)] = {"eval_clustering": R.eval_clustering(torch.from_numpy(x), torch.from_numpy(lab), n_clusters=k),
                         "nearest_other_partition_gap": float(min(gaps)) if gaps else None}
    meta["multiple_k"] = {"case": "set8", "result": mk, "per_k": per_k}

    # kmeans(init=...) level: relocation of two clusters that start empty; a run that stops by tolerance
    def explicit(name, n, d, classes, sep, k, tol, mutate, want_strict):
        seed = 2000
        while True:
            print(name, "seed", seed, flush=True)
            x, _ = small_set(seed, n, d, classes, sep)
            rng = np.random.default_rng(seed + 7)
            init = x[rng.choice(n, size=k, replace=False)].copy()
            mutate(init)
            lab, inertia, n_iter = ref_kmeans(x, k, init=init, n_init=1, tol=tol)
            info, trace = {}, []
            mine = CR.kmeans(x, k, init=init, tol=tol, trace=trace, info=info)
            ok = info["strict"] == want_strict and CR.same_partition(mine["labels"], lab) and mine["n_iter"] == n_iter
            if name == "relocate":
                ok = ok and np.bincount(trace[0], minlength=k).min() == 0 and (np.bincount(trace[0], minlength=k) == 0).sum() == 2
            for s in NOISE_SEEDS:
                ok = ok and CR.same_partition(ref_kmeans(noisy(x, s), k, init=init, n_init=1, tol=tol)[0], lab)
            if ok:
                break
            seed += 1
        out[f"{name}/x"], out[f"{name}/init"], out[f"{name}/km_labels"] = x, init, lab.astype(np.int16)
        meta["cases_init"][name] = {"k": k, "tol": tol, "inertia": inertia, "n_iter": n_iter, "strict": want_strict, "seed": seed}

    meta["cases_init"] = {}

    def displace(init):
        init[1] += 1000.0
        init[4] -= 1000.0
    explicit("relocate", 400, 16, 6, 1.0, 6, 1e-4, displace, True)
    explicit("tol_stop", 900, 16, 5, 0.3, 5, 3e-2, lambda init: None, False)

    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "clustering.npz")
    np.savez_compressed(path, **out)
    print(json.dumps(meta, indent=1))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
