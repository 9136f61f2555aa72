"""Golden generator for the metric kernels past the shapes of clustering.npz / silhouette.npz: rows wider than 1024 columns (1280 =
EfficientNet, 1536 = two concatenated taps), k-means with more clusters than one 128-column assign tile, silhouettes over hundreds of
labels.  Writes tests/golden/metrics_wide.npz.

Run in the development container only (it needs the reference checkout, torch and scikit-learn); nothing under tests/ imports this
module.  It reuses the two generators it extends: make_clustering_goldens.eval_case (the REAL reference's eval_clustering, scikit-learn's
KMeans labels / inertia / n_iter / first-restart seeds, and the stability conditions: the partition survives 1e-6 input noise under three
seeds, no other partition within 1e-5 of the winner's inertia -- a case that fails gets another data seed, meta["max_unstable"] = 0) and
make_silhouette_goldens.check_conditions.  One more condition here, which the longer seeding runs of k = 150 / 200 need: the first
restart's seed rows by the NumPy restatement ARE scikit-learn's.  (With 149 steps of 7 candidates two candidate potentials can tie to
2e-7 relative -- set40_k150 at data seed 1000, step 114 -- and then the rounding of scikit-learn's fp32 GEMM-form distances decides
against the direct differences of the restatement and of the device, and against fp64.)  And one for the assign step, which the
noise check above samples only three times: wherever, on any restart's path, a point's two nearest centres are closer than ASSIGN_ZONE
(relative to ||x||^2 + ||c||^2) -- the zone in which the rounding of an fp32 product sum of D terms decides, about sqrt(D) 2^-24 of its
magnitude, 2e-6 at D = 1280, so 1e-5 leaves 5 x -- that restart is run again with the point given to the other centre, and the winning
partition must still win by MIN_GAP (single_flip_stable).  At D = 1280 and sep 0.08 a dozen such near-ties occur per case; most heal
within an iteration, one at data seed 1000 did not.  Inputs are regenerated in the tests from seeds
(tests/_clustering_ref.clustered, pinned by a SHA-256; tests/_silhouette_ref.WIDE_CASES); the npz holds expected values only:

  meta["cases"], "<case>/km_labels", "<case>/seeds0"      clustering cases, laid out as in clustering.npz
  meta["scores_table"]                                    sklearn.metrics' ARI / NMI / V on a contingency table of hundreds x hundreds of classes
  meta["silhouette"], "sil/<case>/<metric>"               scikit-learn float64 silhouette samples and scores, and the error of the NumPy
                                                          emulation of the device arithmetic against them (the basis of the tests' bars)
  meta["eval_silhouette"]                                 the silhouette score of scikit-learn's k-means partition of the widest clustering case
"""
import json
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _clustering_ref as CR  # noqa: E402
import _silhouette_ref as SR  # noqa: E402
import make_clustering_goldens as GC  # noqa: E402
import make_silhouette_goldens as GS  # noqa: E402

# name -> (n, d, classes, sep, n_clusters)
CLUSTERING = {"wide8_d1280": (1200, 1280, 8, 0.08, None), "wide10_d1536": (1000, 1536, 10, 0.08, None),
              "set40_k150": (1500, 64, 40, 1.0, 150), "set20_k200": (700, 48, 20, 1.0, 200)}
EVAL_SILHOUETTE_CASE = "wide8_d1280"


ASSIGN_ZONE = 1e-5


class AssignProbe:
    """CR.assign with a look at the fp64 distances: records (call, point, second-nearest centre) of every near-tie inside ASSIGN_ZONE, and
    gives the point of `flip` = (call, point, centre) to that centre."""

    def __init__(self, assign, flip=None):
        self.assign, self.flip, self.calls, self.ties = assign, flip, 0, []

    def __call__(self, xc, centres):
        lab, part = self.assign(xc, centres)
        x64, c64 = xc.astype(np.float64), centres.astype(np.float64)
        cn = (c64 ** 2).sum(axis=1)
        full = cn[None, :] - 2.0 * x64 @ c64.T
        order = np.argsort(full, axis=1)[:, :2]
        rows = np.arange(xc.shape[0])
        gap = full[rows, order[:, 1]] - full[rows, order[:, 0]]
        scale = (x64 ** 2).sum(axis=1) + cn[order[:, 0]]
        for p in np.flatnonzero(gap < ASSIGN_ZONE * scale):
            other = order[p, 1] if lab[p] == order[p, 0] else order[p, 0]
            self.ties.append((self.calls, int(p), int(other)))
        if self.flip is not None and self.flip[0] == self.calls:
            _, p, j = self.flip
            lab, part = lab.copy(), part.copy()
            lab[p], part[p] = j, np.float32(full[p, j])
        self.calls += 1
        return lab, part


def single_flip_stable(x, k, mine):
    """Every near-tie of every restart decided the other way, one at a time: the winning partition still wins, by MIN_GAP."""
    xc, _, tol_abs = CR.prepare(x)
    plain = CR.assign
    n_ties = 0
    try:
        for r in range(len(mine["inertias"])):
            CR.assign = probe = AssignProbe(plain)
            base = CR.lloyd(xc, xc[mine["seed_indices"][r]], tol_abs)
            assert np.array_equal(base[0], mine["all_labels"][r])
            n_ties += len(probe.ties)
            for flip in probe.ties:
                CR.assign = AssignProbe(plain, flip)
                lab, _, inertia, _ = CR.lloyd(xc, xc[mine["seed_indices"][r]], tol_abs)
                labels = list(mine["all_labels"])
                inertias = np.array(mine["inertias"], dtype=np.float64)
                labels[r], inertias[r] = lab, inertia
                best = int(np.argmin(inertias))
                other = [i for i, l in zip(inertias, labels) if not CR.same_partition(l, labels[best])]
                if not CR.same_partition(labels[best], mine["labels"]) or (other and min(other) < inertias[best] * (1.0 + GC.MIN_GAP)):
                    print("   restart", r, "near-tie", flip, "decided the other way changes the winner: inertia", inertia)
                    return None
    finally:
        CR.assign = plain
    return n_ties


def main():
    import sklearn
    from sklearn import metrics
    warnings.filterwarnings("ignore")
    R = GC.load_reference()
    out, meta = {}, {"sklearn": sklearn.__version__, "noise": GC.NOISE, "noise_seeds": list(GC.NOISE_SEEDS), "min_gap": GC.MIN_GAP,
                     "max_unstable": 0, "cases": {}}

    for name, (n, d, classes, sep, n_clusters) in CLUSTERING.items():
        seed = 1000
        while True:
            print(name, "seed", seed, flush=True)
            x, lab = CR.clustered(seed, n, d, classes, sep)
            got = GC.eval_case(R, x, lab, n_clusters, gen={"seed": seed, "n": n, "d": d, "classes": classes, "sep": sep}, store_x=False)
            if got is not None:
                mine = CR.kmeans(x, got[1]["k"])
                if not np.array_equal(mine["seed_indices"][0], got[0]["seeds0"]):
                    print("   the first restart's seed rows differ from scikit-learn's at step", int(np.flatnonzero(mine["seed_indices"][0] != got[0]["seeds0"])[0]))
                else:
                    n_ties = single_flip_stable(x, got[1]["k"], mine)
                    if n_ties is not None:
                        break
            seed += 1
        arrays, m = got
        arrays.pop("labels")
        m["assign_near_ties_survived"], m["assign_zone"] = n_ties, ASSIGN_ZONE
        m["restatement_n_iter"] = int(mine["n_iter"])
        m["restatement_same_partition"] = bool(CR.same_partition(mine["labels"], arrays["km_labels"]))
        for key, a in arrays.items():
            out[f"{name}/{key}"] = a
        meta["cases"][name] = m
        print(name, json.dumps(m), flush=True)

    # the three scores on a table of about 300 x 350 occupied classes
    g = CR.SCORES_TABLE
    a, b = CR.label_pair(**g)
    meta["scores_table"] = {"gen": g, "classes_true": int(np.unique(a).size), "classes_pred": int(np.unique(b).size), "sha256": CR.sha256(a, b),
                            "ari": float(metrics.adjusted_rand_score(a, b)), "nmi": float(metrics.normalized_mutual_info_score(a, b)),
                            "v_measure": float(metrics.v_measure_score(a, b))}
    print("scores_table", json.dumps(meta["scores_table"]), flush=True)

    meta["silhouette"] = {"tol_sample": SR.TOL_SAMPLE, "tol_score": SR.TOL_SCORE, "mfma_margin": SR.MFMA_MARGIN, "cases": {}}
    for name in SR.WIDE_CASES:
        x, lab = SR.case_inputs(name)
        assert x.dtype == np.float32
        m = {"n": int(x.shape[0]), "d": int(x.shape[1]), "k": int(np.unique(lab).size), "conditions": GS.check_conditions(name, x), "score": {},
             "restatement_max_err": {}, "restatement_score_err": {}}
        for metric in SR.METRICS:
            s = metrics.silhouette_samples(x.astype(np.float64), lab, metric=metric)
            out[f"sil/{name}/{metric}"] = s.astype(np.float64)
            m["score"][metric] = float(metrics.silhouette_score(x.astype(np.float64), lab, metric=metric))
            mine = SR.silhouette_samples(x, lab, metric)
            m["restatement_max_err"][metric] = float(np.abs(mine - s).max())
            m["restatement_score_err"][metric] = abs(float(mine.sum() / mine.shape[0]) - m["score"][metric])
        meta["silhouette"]["cases"][name] = m
        print(name, json.dumps(m), flush=True)

    # the Euclidean silhouette of scikit-learn's k-means partition of the widest clustering case: what eval_clustering_silhouette adds
    c = meta["cases"][EVAL_SILHOUETTE_CASE]
    x, _ = CR.clustered(**c["gen"])
    km = out[f"{EVAL_SILHOUETTE_CASE}/km_labels"].astype(np.int64)
    score = float(metrics.silhouette_score(x.astype(np.float64), km, metric="euclidean"))
    meta["eval_silhouette"] = {"case": EVAL_SILHOUETTE_CASE, "score": score, "restatement_score_err": {"euclidean": abs(SR.silhouette_score(x, km) - score)},
                               "restatement_max_err": {"euclidean": float(np.abs(SR.silhouette_samples(x, km) - metrics.silhouette_samples(
                                   x.astype(np.float64), km, metric="euclidean")).max())}}
    print("eval_silhouette", json.dumps(meta["eval_silhouette"]), flush=True)

    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "metrics_wide.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
