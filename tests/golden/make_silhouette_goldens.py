"""Golden generator for the device silhouette: scikit-learn's silhouette_samples / silhouette_score on a FLOAT64 copy of the fp32
inputs, for both metrics, written to tests/golden/silhouette.npz.  (scikit-learn's own float32 path rounds the distances to fp32 and
sits 1.1e-7 .. 1.7e-7 per sample from its float64 path: the worse yardstick.)

Run where scikit-learn is installed; nothing under tests/ imports this module.  The inputs are regenerated from seeds by
tests/_silhouette_ref.py (CASES, SAMPLED); only expected values are stored.

Conditions a case must meet, so that the reference alone stays inside the tolerances (asserted here):
  * no two distinct rows are closer than 1e-2 of the set's RMS centred norm, unless they are bit-identical: the fp32 Gram form loses
    the distance of near-duplicates (its absolute error is about 1e-7 ||x||^2 in the SQUARE of the distance);
  * the mean pairwise cosine distance of a set is >= 0.5: a dominant common direction degrades fp32 cosine distances, and
    scikit-learn's own fp32 path with them, to about 3e-6 per sample.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _silhouette_ref as SR  # noqa: E402

MIN_SEPARATION, MIN_MEAN_COSINE_DISTANCE = 1e-2, 0.5


def check_conditions(name, x):
    from sklearn.metrics import pairwise_distances
    x64 = x.astype(np.float64)
    xc = x64 - x64.mean(axis=0)
    rms = float(np.sqrt((xc ** 2).sum(axis=1).mean()))
    d = pairwise_distances(xc)
    same = (x[:, None, 0] == x[None, :, 0])
    for i, j in zip(*np.nonzero(same)):
        same[i, j] = np.array_equal(x[i], x[j])
    d[same] = np.inf
    sep = float(d.min() / rms)
    cos = pairwise_distances(x64, metric="cosine")
    mean_cos = float(cos[~np.eye(len(x), dtype=bool)].mean())
    assert sep >= MIN_SEPARATION, (name, sep)
    assert mean_cos >= MIN_MEAN_COSINE_DISTANCE, (name, mean_cos)
    return {"min_separation_over_rms": sep, "mean_cosine_distance": mean_cos, "identical_pairs": int((same.sum() - len(x)) // 2)}


def main():
    import sklearn
    from sklearn.metrics import silhouette_samples, silhouette_score
    out, meta = {}, {"sklearn": sklearn.__version__, "tol_sample": SR.TOL_SAMPLE, "tol_score": SR.TOL_SCORE, "min_separation": MIN_SEPARATION,
                     "min_mean_cosine_distance": MIN_MEAN_COSINE_DISTANCE, "cases": {}, "sampled": []}
    for name in SR.CASES:
        x, lab = SR.case_inputs(name)
        assert x.dtype == np.float32
        m = {"n": int(x.shape[0]), "d": int(x.shape[1]), "k": int(np.unique(lab).size), "conditions": check_conditions(name, x), "score": {}}
        for metric in SR.METRICS:
            s = silhouette_samples(x.astype(np.float64), lab, metric=metric)
            out[f"{name}/{metric}"] = s.astype(np.float64)
            m["score"][metric] = float(silhouette_score(x.astype(np.float64), lab, metric=metric))
            mine = SR.silhouette_samples(x, lab, metric)
            m.setdefault("restatement_max_err", {})[metric] = float(np.abs(mine - s).max())
        meta["cases"][name] = m
        print(name, json.dumps(m), flush=True)
    for name, draws in SR.SAMPLED.items():
        x, lab = SR.case_inputs(name)
        for size, seed in draws:
            idx = SR.sample_indices(x.shape[0], size, seed)
            rec = {"case": name, "sample_size": size, "random_state": seed, "score": {}}
            for metric in SR.METRICS:
                rec["score"][metric] = float(silhouette_score(x.astype(np.float64), lab, metric=metric, sample_size=size, random_state=seed))
                out[f"{name}/sample{size}_seed{seed}/{metric}"] = silhouette_samples(x[idx].astype(np.float64), lab[idx], metric=metric)
            out[f"{name}/sample{size}_seed{seed}/indices"] = idx.astype(np.int32)
            meta["sampled"].append(rec)
            print(json.dumps(rec), flush=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "silhouette.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
