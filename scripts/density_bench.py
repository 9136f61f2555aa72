#!/usr/bin/env python3
"""Device time of density clustering (avex_amd.density) on the MI355X:

  (a) one count pass and one hook pass over 65 536 x 768 rows (the O(N^2 D) passes: their time does not depend on the data);
  (b) rounds and total time on embeddings-like planted data: 64 call types of 512 windows each (relative noise 0.05 around unit-normal
      centres) among as many background rows, eps 0.01, min_samples 5;
  (c) rounds and total time on a path of 4 096 rows in shuffled order (eps 4e-4, min_samples 3): the longest chain of core rows a set of
      that size can hold, which plain min-label propagation would need thousands of passes for.

    python scripts/density_bench.py [--rows 65536] [--dim 768] [--out profiles/density_bench.json]

Total times are wall-clock around dbscan() after one warm-up (the function synchronises once per round), best of three; pass times are
events around the launches of one pass (the `_timing` switch of dbscan)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import density  # noqa: E402
from avex_amd.search import EmbeddingIndex  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9      # 157 TF: DESIGN.md 4.11a


def run(x, eps, min_samples, reps=3):
    """(result, best wall-clock seconds, pass times of the best run)"""
    density.dbscan(x, eps, min_samples)
    best, split, res = float("inf"), None, None
    for _ in range(reps):
        t = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = density.dbscan(x, eps, min_samples, _timing=t)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt < best:
            best, split = dt, t
    return res, best, split


def path(n, step=0.02 * np.sqrt(2.0), turn=5e-4):
    """n points whose neighbours in the list are at cosine distance 2e-4 and whose next neighbours are at 8e-4: two rotations, a fast one
    (the path) and a slow one that never closes (it keeps the turns of the fast one apart)."""
    k = np.arange(n, dtype=np.float64)
    return np.stack([np.cos(step * k), np.sin(step * k), np.cos(turn * k), np.sin(turn * k)], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, d = a.rows, a.dim
    g = torch.Generator(device="cuda").manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "d": d}

    types, per = 64, n // 128
    centres = torch.randn(types, d, device="cuda", generator=g)
    calls = centres.repeat_interleave(per, dim=0) * (1.0 + 0.05 * torch.randn(types * per, d, device="cuda", generator=g))
    x = torch.cat([calls, torch.randn(n - types * per, d, device="cuda", generator=g)])
    x = x[torch.randperm(n, device="cuda", generator=g)]
    ix = EmbeddingIndex(d)
    ix.add(x)
    res, total, split = run(ix, 0.01, 5)
    flops = 2.0 * n * n * d
    hook = min(split["hook_s"])
    out["passes"] = {"count_pass_s": split["count_s"], "hook_pass_s": hook, "count_tflops": flops / split["count_s"] / 1e12,
                     "hook_tflops": flops / hook / 1e12, "count_share_of_fp32_mfma_peak": flops / split["count_s"] / PEAK_F32_MFMA}
    sizes = res["sizes"].cpu().numpy()
    out["planted"] = {"call_types": types, "rows_per_type": per, "eps": 0.01, "min_samples": 5, "rounds": res["rounds"], "total_s": total,
                      "n_clusters": res["n_clusters"], "largest": int(sizes.max()) if len(sizes) else 0, "noise": int((res["labels"] < 0).sum())}
    print(json.dumps(out), flush=True)
    del ix, x, calls

    p = path(4096)
    p = p[np.random.RandomState(0).permutation(len(p))]
    res, total, split = run(p, 4e-4, 3)
    assert res["n_clusters"] == 1 and int(res["core"].sum()) == 4094, (res["n_clusters"], int(res["core"].sum()))
    out["path"] = {"rows": 4096, "eps": 4e-4, "min_samples": 3, "rounds": res["rounds"], "total_s": total, "n_clusters": res["n_clusters"],
                   "hook_pass_s": min(split["hook_s"])}
    print(json.dumps(out["path"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
