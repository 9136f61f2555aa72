#!/usr/bin/env python3
"""Device time of the silhouette score (avex_amd.clustering.silhouette_score) at N = 65 536 x D = 768 with 64 and 512 labels, both metrics.

    python scripts/silhouette_bench.py [--n 65536] [--dim 768] [--labels 64,512] [--cpu-n 16384] [--cpu-labels 64] [--out profiles/silhouette_bench.json]

Per (labels, metric) (one warm-up, then --reps timed repeats; min / median / max are recorded):
  * silhouette_score end to end (events around the call: centring or normalising, label densification, the cluster-ordered layout, every
    batch, the read-back), and one call with the stages launched apart (prepare, the distance product with its per-cluster sums, the
    per-point pass and the mean);
  * the product stage of every batch (avexhip_silhouette_batch, stages = 1) against retr_sim_kernel on the same product shape in the same
    process -- the same number of batches of 2048 rows against the same number of rows, through avexhip_retrieval_batch stage 1 (self-set:
    no query normalisation) -- and both as a share of the fp32 MFMA peak (256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz = 157 TF).
CPU leg (--cpu-n 0 skips it): scikit-learn's silhouette_score on this machine's CPUs, where it can be imported, against the device on the
same inputs, with both scores."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import _capi  # noqa: E402
from avex_amd import clustering as K  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9
BATCH = 2048


def make(n, d, classes, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, classes, (n,), device="cuda", generator=g)
    x = torch.randn(n, d, device="cuda", generator=g) + 0.15 * torch.randn(classes, d, device="cuda", generator=g)[lab]
    return x, lab


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return {"min_s": min(out), "median_s": statistics.median(out), "max_s": max(out), "max_minus_min_s": max(out) - min(out), "reps": reps}


def product_ab(x, lab, metric, reps):
    """Stage 1 of every batch against retr_sim_kernel on the same product shape."""
    lib = _capi.lib()
    n, d = x.shape
    dev = x.device
    s = K._stream()
    ids, n_labels = K._dense_ids(lab, dev)
    slot_src, group, counts, n_slots = K._sil_layout(ids, n_labels, dev)
    nbytes = int(lib.avexhip_silhouette_workspace_bytes(n_slots, d, n_labels, BATCH))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    samples = torch.zeros((n,), dtype=torch.float64, device=dev)
    a = _capi.SilhouetteArgs()
    a.x, a.ld_x, a.n, a.d, a.metric, a.n_labels, a.n_slots, a.batch = x.data_ptr(), x.stride(0), n, d, K._SIL_METRICS[metric], n_labels, n_slots, BATCH
    a.slot_src, a.group_label, a.counts = slot_src.data_ptr(), group.data_ptr(), counts.data_ptr()
    a.workspace, a.workspace_bytes, a.samples_out, a.stages = ws.data_ptr(), nbytes, samples.data_ptr(), 1
    _capi.check(lib.avexhip_silhouette_prepare(C.byref(a), s), "silhouette_prepare")
    starts = list(range(0, n_slots, BATCH))

    def product():
        for row0 in starts:
            a.row0, a.nb = row0, min(BATCH, n_slots - row0)
            _capi.check(lib.avexhip_silhouette_batch(C.byref(a), s), "silhouette_batch")

    t_prod = timed(product, reps)
    del ws
    # the yardstick: the same batches of rows against the same n_slots rows
    db = torch.randn(n_slots, d, device=dev)
    ws_bytes = int(lib.avexhip_retrieval_workspace_bytes(n_slots, d, BATCH, 0))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _capi.check(lib.avexhip_retrieval_prepare(db.data_ptr(), db.stride(0), n_slots, d, BATCH, ws.data_ptr(), ws_bytes, s), "retrieval_prepare")
    zeros = torch.zeros((n_slots,), dtype=torch.int32, device=dev)
    r = _capi.RetrievalArgs()
    r.query, r.ld_query, r.n_db, r.d, r.batch, r.n_words, r.self_set, r.k, r.stages = None, 0, n_slots, d, BATCH, 0, 1, 1, 1
    r.query_ids, r.db_ids, r.workspace, r.workspace_bytes = zeros.data_ptr(), zeros.data_ptr(), ws.data_ptr(), ws_bytes
    u2 = torch.empty((BATCH,), dtype=torch.int64, device=dev)
    st = torch.empty((BATCH, 4), dtype=torch.int32, device=dev)
    tk = torch.empty((BATCH, 32), dtype=torch.int32, device=dev)
    r.u2, r.stats, r.topk = u2.data_ptr(), st.data_ptr(), tk.data_ptr()

    def sim():
        for row0 in starts:
            r.q0, r.nb = row0, min(BATCH, n_slots - row0)
            _capi.check(lib.avexhip_retrieval_batch(C.byref(r), s), "retrieval_batch")

    t_sim = timed(sim, reps)
    flops = 2.0 * n_slots * n_slots * d
    return {"n_slots": n_slots, "batches": len(starts), "flops": flops, "silhouette_product_stage": t_prod, "retr_sim_stage1": t_sim,
            "product_over_retr_sim": t_prod["median_s"] / t_sim["median_s"],
            "product_share_of_fp32_mfma_peak": flops / t_prod["median_s"] / PEAK_F32_MFMA,
            "retr_sim_share_of_fp32_mfma_peak": flops / t_sim["median_s"] / PEAK_F32_MFMA}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--labels", default="64,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=16384)
    ap.add_argument("--cpu-labels", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for k in [int(s) for s in a.labels.split(",") if s]:
        x, lab = make(a.n, a.dim, k)
        for metric in ("euclidean", "cosine"):
            res = {}
            total = timed(lambda: res.update(score=K.silhouette_score(x, lab, metric=metric)), a.reps)
            split = {}
            K.silhouette_score(x, lab, metric=metric, _timing=split)
            row = {"n": a.n, "d": a.dim, "labels": k, "metric": metric, "batch_size": BATCH, "silhouette_score": total, "score": res["score"],
                   "stages_of_one_call": split, "product_ab": product_ab(x, lab, metric, a.reps)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x, lab
        torch.cuda.empty_cache()
    cpu = None
    if a.cpu_n > 0:
        x, lab = make(a.cpu_n, a.dim, a.cpu_labels)
        cpu = {"n": a.cpu_n, "d": a.dim, "labels": a.cpu_labels, "cpu_threads": torch.get_num_threads(), "metrics": {}}
        for metric in ("euclidean", "cosine"):
            dev = timed(lambda: K.silhouette_score(x, lab, metric=metric), a.reps)
            leg = {"device_silhouette_score": dev, "device_score": K.silhouette_score(x, lab, metric=metric)}
            try:
                from sklearn.metrics import silhouette_score
                xh, lh = x.cpu().numpy(), lab.cpu().numpy()
                t0 = time.perf_counter()
                leg["sklearn_score_fp32_input"] = float(silhouette_score(xh, lh, metric=metric))
                leg["sklearn_s"] = time.perf_counter() - t0
                leg["sklearn_over_device"] = leg["sklearn_s"] / dev["median_s"]
                leg["score_difference"] = abs(leg["sklearn_score_fp32_input"] - leg["device_score"])
                cpu["sklearn_where"] = "this machine"
            except ImportError:
                cpu["sklearn_where"] = "not importable on this machine"
            cpu["metrics"][metric] = leg
        print(json.dumps(cpu), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "sizes": rows, "cpu_leg": cpu}, f, indent=1)


if __name__ == "__main__":
    main()
