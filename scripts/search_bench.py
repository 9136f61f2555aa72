#!/usr/bin/env python3
"""Device time of a query-by-example search (avex_amd.search) at 10^5, 10^6 and 4 x 10^6 rows x 768, 1 024 queries, k in {10, 100, 1024},
with and without temporal suppression, split into similarity, select and finish; and, on the same tensors, torch.topk(q @ db.T, k) in
fp32 as the yardstick where its [queries, rows] matrix fits in memory.

    python scripts/search_bench.py [--sizes 100000,1000000,4000000] [--ks 10,100,1024] [--queries 1024] [--out profiles/search_bench.json]

Per size and k: the whole search (events around the call, one warm-up), and every chunk's similarity and select stage and every batch's
finish launched separately with events between them (the `stages` switch of avexhip_search_chunk).  The rows carry synthetic recordings
of 1 000 windows with hop = window / 4, so the suppression has something to do.  The torch leg holds the database as one [rows, 768]
tensor next to the index; a shape whose product would not fit is reported as "torch_s": null with the reason."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import search as S  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9


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


def build(n, d, chunk_rows, piece=1 << 18, seed=0):
    """An index of n random rows, generated and added piece by piece (the full [n, d] tensor is only made for the torch leg)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ix = S.EmbeddingIndex(d, chunk_rows=chunk_rows)
    for lo in range(0, n, piece):
        m = min(piece, n - lo)
        rows = torch.arange(lo, lo + m, device="cuda")
        start = (rows % 1000).double() * 0.25
        ix.add(torch.randn(m, d, device="cuda", generator=g), recording=(rows // 1000).int(), start_s=start, end_s=start + 1.0)
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--ks", default="10,100,1024")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = []
    for n in [int(s) for s in a.sizes.split(",") if s]:
        ix = build(n, a.dim, a.chunk_rows)
        q = torch.randn(a.queries, a.dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        flops = 2.0 * n * a.queries * a.dim
        for k in [int(s) for s in a.ks.split(",") if s]:
            for nms in (None, 0.5):
                kw = dict(nms=nms, batch_size=a.batch_size)
                total = timed(lambda: ix.search(q, k, **kw))
                split = {}
                ix.search(q, k, _timing=split, **kw)
                ix.search(q, k, _timing=split, **kw)
                row = {"n": n, "d": a.dim, "queries": a.queries, "k": k, "nms": nms, "list_depth": k if nms is None else min(4 * k, S.MAX_K),
                       "chunk_rows": a.chunk_rows, "total_s": total, **split, "similarity_tflops": flops / split["similarity_s"] / 1e12,
                       "similarity_share_of_fp32_mfma_peak": flops / split["similarity_s"] / PEAK_F32_MFMA}
                out.append(row)
                print(json.dumps(row), flush=True)
        # the yardstick: normalised rows as one tensor, one product, one topk
        free = torch.cuda.mem_get_info()[0]
        need = 4 * n * (a.dim + 2 * a.queries)          # the database copy, the product, and topk's scratch of about its size
        if need > 0.9 * free:
            for k in [int(s) for s in a.ks.split(",") if s]:
                row = {"n": n, "k": k, "torch_s": None, "reason": f"needs about {need / 2 ** 30:.1f} GiB beside the index, {free / 2 ** 30:.1f} GiB free"}
                out.append(row)
                print(json.dumps(row), flush=True)
        else:
            db = torch.cat([c[:min(ix.chunk_rows, n - i * ix.chunk_rows), :a.dim] for i, c in enumerate(ix._chunks)])
            qn = torch.nn.functional.normalize(q, dim=1)
            for k in [int(s) for s in a.ks.split(",") if s]:
                t = timed(lambda: torch.topk(qn @ db.T, k, dim=1))
                row = {"n": n, "k": k, "torch_s": t}
                out.append(row)
                print(json.dumps(row), flush=True)
            del db
        del ix
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
