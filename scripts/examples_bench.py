#!/usr/bin/env python3
"""Device time of few-shot scoring (avex_amd.examples) of 2^20 windows x 768 against (a) 50 classes x 5 examples and (b) 200 classes x 50
examples plus 10 000 background rows, top_m in {1, 5}, split into the tile and the reduce stage; and, on the same tensors, the
composition torch offers without the fused kernel as the yardstick: q @ bank.T over query batches that fit, then topk per class on the
class-sorted columns.

    python scripts/examples_bench.py [--windows 1048576] [--top-ms 1,5] [--batch-size 4096] [--out profiles/examples_bench.json]

Per bank and top_m: the whole score (events around the call, one warm-up, best of three), and every batch's tile and reduce stage
launched separately with events between them (the `stages` switch of avexhip_examples_score).  The torch leg reads the bank's own
class-sorted prepared rows and queries normalised once outside the timed region; equal-sized classes let it take one topk over a
[batch, classes, rows] view, which is the fastest form it has."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import examples as X  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9      # 157 TF: DESIGN.md 4.11a


def timed(fn, reps=3):
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


def torch_scores(qn, bank, n_classes, per_class, n_bg, top_m, margin, batch):
    """scores [N, C] the torch way: per query batch the [batch, M] product, then the top_m mean per class (and the background's)."""
    out = torch.empty((qn.shape[0], n_classes), dtype=torch.float32, device=qn.device)
    m_cls = n_classes * per_class
    for lo in range(0, qn.shape[0], batch):
        s = qn[lo:lo + batch] @ bank.T
        v = s[:, :m_cls].view(-1, n_classes, per_class).topk(min(top_m, per_class), dim=2).values.mean(dim=2)
        if margin:
            v = v - s[:, m_cls:].topk(min(top_m, n_bg), dim=1).values.mean(dim=1, keepdim=True)
        out[lo:lo + batch] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--top-ms", default="1,5")
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--torch-batch", type=int, default=32768)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(a.windows, a.dim, device="cuda", generator=g)
    qn = torch.nn.functional.normalize(q, dim=1)
    out = []
    for name, n_classes, per_class, n_bg in (("a: 50 classes x 5", 50, 5, 0), ("b: 200 classes x 50 + 10000 background", 200, 50, 10000)):
        labels = np.concatenate([np.repeat(np.arange(n_classes), per_class), np.full(n_bg, -1)])
        labels = labels[np.random.RandomState(0).permutation(len(labels))]
        bank = X.ExampleBank(a.dim)
        bank.add(torch.randn(len(labels), a.dim, device="cuda", generator=g), labels)
        mode = "margin" if n_bg else "similarity"
        flops = 2.0 * len(labels) * a.windows * a.dim
        sorted_rows = bank._prepare()["bank"][:, :a.dim].contiguous()
        for top_m in [int(s) for s in a.top_ms.split(",") if s]:
            kw = dict(top_m=top_m, mode=mode, batch_size=a.batch_size)
            total = timed(lambda: bank.score(q, **kw))
            best = {}
            for rep in range(4):                                                # one warm-up, best of three
                split = {}
                bank.score(q, _timing=split, **kw)
                if rep:
                    best = {k: min(v, best.get(k, v)) for k, v in split.items()}
            t_torch = timed(lambda: torch_scores(qn, sorted_rows, n_classes, per_class, n_bg, top_m, bool(n_bg), a.torch_batch))
            ours = bank.score(q[:4096], **kw)
            ref = torch_scores(qn[:4096], sorted_rows, n_classes, per_class, n_bg, top_m, bool(n_bg), 4096)
            row = {"bank": name, "rows": len(labels), "segments": bank._prepare()["n_segments"], "windows": a.windows, "d": a.dim, "top_m": top_m, "mode": mode,
                   "batch_size": a.batch_size, "total_s": total, **best, "tile_tflops": flops / best["tile_s"] / 1e12,
                   "tile_share_of_fp32_mfma_peak": flops / best["tile_s"] / PEAK_F32_MFMA, "torch_s": t_torch, "torch_batch": a.torch_batch,
                   "torch_over_fused": t_torch / total, "max_abs_difference_to_torch": float((ours - ref).abs().max())}
            out.append(row)
            print(json.dumps(row), flush=True)
        del bank, sorted_rows
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
