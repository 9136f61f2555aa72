"""Golden generator for avex_amd.density: sklearn.cluster.DBSCAN(algorithm="brute") on a FLOAT64 copy of the planted fp32 inputs of
tests/_density_ref.py (CASES), both metrics, written to tests/golden/density.npz: per case the labels, the core rows and eps.

Run where scikit-learn is installed; nothing under tests/ imports this module.  The inputs are regenerated from synth names; only eps
and the expected values are stored.  eps sits in the middle of the widest gap of the sorted pairwise distances near their 5 % quantile
(_density_ref.gap_eps); the gap is asserted here against the same floors the CPU test asserts, so that no pair sits at the threshold.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _density_ref as D  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import DBSCAN
    out, meta = {}, {"sklearn": sklearn.__version__, "min_samples": D.MIN_SAMPLES, "cases": {}}
    for n, d in D.CASES:
        x = D.planted(D.case_name(n, d), n, d)
        for metric in D.METRICS:
            eps, gap = D.gap_eps(x, metric)
            assert gap >= D.MIN_GAP[metric], (n, d, metric, gap)
            fit = DBSCAN(eps=eps, min_samples=D.MIN_SAMPLES, metric=metric, algorithm="brute").fit(x.astype(np.float64))
            key = f"{D.case_name(n, d)}/{metric}"
            out[f"{key}/labels"] = fit.labels_.astype(np.int32)
            out[f"{key}/core"] = np.sort(fit.core_sample_indices_).astype(np.int32)
            out[f"{key}/eps"] = np.asarray(eps, dtype=np.float64)
            meta["cases"][key] = {"eps": eps, "gap": gap, "clusters": int(fit.labels_.max() + 1), "noise": int((fit.labels_ < 0).sum()),
                                  "core": int(len(fit.core_sample_indices_))}
            print(key, json.dumps(meta["cases"][key]), flush=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "density.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
