#!/usr/bin/env python3
"""Device time of the retrieval metrics (avex_amd.retrieval) at N = 8 Ki, 32 Ki, 64 Ki x D = 768, split into similarity and rank, and
the reference-style CPU time (one fp32 NumPy product per batch + one rank statistic per query) at the largest N one is willing to wait for.

    python scripts/retrieval_bench.py [--sizes 8192,32768,65536] [--classes 50] [--cpu-n 1536] [--out profiles/retrieval_bench.json]

Per size: whole eval_retrieval time (events around the call, one warm-up; label preparation included), and the similarity and the rank
stage of every batch launched separately with events between them (the `stages` switch of avexhip_retrieval_batch), the similarity kernel's share of the fp32 MFMA peak (256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz = 157 TF),
and the rank kernel's modelled LDS reads: every ranked item of the larger side does ceil(log2 min(P, Q)) + 1 probes of the sorted smaller
side (a second search only on an exact tie), against the N log2 min(P, Q) model.  --cpu-n 0 skips the CPU leg; with scikit-learn
present it calls roc_auc_score per query like the reference, without it the same rank statistic in NumPy."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import retrieval as R  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9


def make(n, d, classes, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, classes, (n,), device="cuda", generator=g)
    x = torch.randn(n, d, device="cuda", generator=g) + 0.15 * torch.randn(classes, d, device="cuda", generator=g)[lab]
    return x, lab


def timed(fn, reps=2):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def cpu_reference_style(x, lab, batch=2048):
    """What avex/evaluation/retrieval.py does for eval_retrieval's AUC half: fp32 product per batch, one AUC per query in a Python loop."""
    try:
        from sklearn.metrics import roc_auc_score
    except Exception:  # noqa: BLE001
        roc_auc_score = None
    normed = x / np.linalg.norm(x, axis=1, keepdims=True).clip(1e-12)
    n = x.shape[0]
    aucs = []
    t0 = time.perf_counter()
    for b0 in range(0, n, batch):
        sim = normed[b0:b0 + batch] @ normed.T
        for i in range(b0, min(b0 + batch, n)):
            y = lab == lab[i]
            if y.sum() <= 1:
                continue
            m = np.ones(n, dtype=bool)
            m[i] = False
            s, r = sim[i - b0][m], y[m]
            if r.all():
                continue
            if roc_auc_score is not None:
                aucs.append(roc_auc_score(r, s))
            else:
                neg = np.sort(s[~r])
                pos = s[r]
                aucs.append((np.searchsorted(neg, pos, "left").sum() + np.searchsorted(neg, pos, "right").sum()) / (2.0 * pos.size * neg.size))
    return time.perf_counter() - t0, float(np.mean(aucs)), roc_auc_score is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,32768,65536")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--cpu-n", type=int, default=1536)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for n in [int(s) for s in a.sizes.split(",") if s]:
        x, lab = make(n, a.dim, a.classes)
        res = {}
        total = timed(lambda: res.update(R.eval_retrieval(x, lab, batch_size=a.batch_size)))
        split = {}
        R.retrieval_stats(x, lab, batch_size=a.batch_size, _timing=split)
        st = R.retrieval_stats(x, lab, batch_size=a.batch_size, _timing=split)
        t_sim, t_rank = split["similarity_s"], split["rank_s"]
        small = torch.minimum(st["n_pos"], st["n_neg"]).double().clamp(min=1)
        large = torch.maximum(st["n_pos"], st["n_neg"]).double()
        probes = float((large * (torch.ceil(torch.log2(small)) + 1)).sum())
        model = float(n) * float(torch.log2(small).sum())
        flops = 2.0 * n * n * a.dim
        row = {"n": n, "d": a.dim, "classes": a.classes, "batch_size": a.batch_size, "total_s": total, "similarity_s": t_sim, "rank_s": t_rank,
               "similarity_tflops": flops / t_sim / 1e12, "similarity_share_of_fp32_mfma_peak": flops / t_sim / PEAK_F32_MFMA,
               "rank_lds_probes": probes, "rank_lds_probes_model_n_log2_min_pq": model, "rank_probe_rate_per_s": probes / max(t_rank, 1e-9), **res}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, lab, st
        torch.cuda.empty_cache()
    cpu = None
    if a.cpu_n > 0:
        x, lab = make(a.cpu_n, a.dim, a.classes)
        sec, auc, sk = cpu_reference_style(x.cpu().numpy(), lab.cpu().numpy())
        dev = timed(lambda: R.evaluate_auc_roc_batched(x, lab))
        cpu = {"n": a.cpu_n, "d": a.dim, "cpu_s": sec, "cpu_auc": auc, "cpu_uses_sklearn": sk, "device_s": dev, "device_auc": R.evaluate_auc_roc_batched(x, lab),
               "cpu_threads": torch.get_num_threads()}
        print(json.dumps(cpu), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "sizes": rows, "cpu_leg": cpu}, f, indent=1)


if __name__ == "__main__":
    main()
