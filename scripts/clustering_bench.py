#!/usr/bin/env python3
"""Device time of the clustering metrics (avex_amd.clustering) at N = 65 536 x D = 768, k = 64 and k = 512.

    python scripts/clustering_bench.py [--n 65536] [--dim 768] [--ks 64,512] [--cpu-n 16384] [--cpu-k 64] [--out profiles/clustering_bench.json]

Per k (one warm-up, then --reps timed repeats; min / median / max are recorded):
  * eval_clustering end to end (events around the call; label preparation, random draws and the polls included), and the stages of one
    kmeans call launched separately with events between them (seeding, the assign product, everything after it);
  * the assign stage with every restart live (first iteration), against retr_sim_kernel (retrieval.hip) on the same box and the same
    product shape -- the R * kpad centre rows as queries against the N data rows, through avexhip_retrieval_batch stage 1 -- and its share
    of the fp32 MFMA peak (256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz = 157 TF);
  * lock-step (n_init = 10 in one call) against the same kernels driven one restart at a time (n_init = 1 ten times on one RandomState:
    the same ten restarts).
CPU leg (--cpu-n 0 skips it): scikit-learn's KMeans with the reference's arguments on this machine's CPUs, where it can be imported,
against the device on the same inputs."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import _capi  # noqa: E402
from avex_amd import clustering as K  # noqa: E402

PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9


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
    return {"min_s": min(out), "median_s": statistics.median(out), "max_s": max(out), "reps": reps}


def assign_ab(x, k, reps):
    """The assign stage of the first iteration (every restart live) and retr_sim_kernel on the same product shape."""
    lib = _capi.lib()
    n, d = x.shape
    prep = K._Prepared(x, k, 10, 1e-4)
    a = prep.args(k, 300)
    s = K._stream()
    first, u = K._draws(n, k, 10, 42)
    fd, ud = torch.from_numpy(first).cuda(), torch.from_numpy(u.reshape(-1)).cuda()
    _capi.check(lib.avexhip_clustering_seed(C.byref(a), fd.data_ptr(), ud.data_ptr(), s), "clustering_seed")
    t_assign = timed(lambda: _capi.check(lib.avexhip_clustering_iterate(C.byref(a), 1, 1, None, s), "clustering_iterate"), reps)
    # the yardstick: R * kpad rows (what the assign product multiplies) as queries against the N data rows
    kpad = (k + 31) // 32 * 32
    nq = 10 * kpad
    q = torch.randn(nq, d, device="cuda")
    ws_bytes = int(lib.avexhip_retrieval_workspace_bytes(n, d, nq, 0))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    _capi.check(lib.avexhip_retrieval_prepare(x.data_ptr(), x.stride(0), n, d, nq, ws.data_ptr(), ws_bytes, s), "retrieval_prepare")
    ids = torch.zeros((max(n, nq),), dtype=torch.int32, device="cuda")
    r = _capi.RetrievalArgs()
    r.query, r.ld_query, r.nb, r.q0, r.n_db, r.d, r.batch, r.n_words, r.self_set, r.k, r.stages = q.data_ptr(), q.stride(0), nq, 0, n, d, nq, 0, 0, 1, 1
    r.query_ids, r.db_ids, r.workspace, r.workspace_bytes = ids.data_ptr(), ids.data_ptr(), ws.data_ptr(), ws_bytes
    u2 = torch.empty((nq,), dtype=torch.int64, device="cuda")
    st = torch.empty((nq, 4), dtype=torch.int32, device="cuda")
    tk = torch.empty((nq, 32), dtype=torch.int32, device="cuda")
    r.u2, r.stats, r.topk = u2.data_ptr(), st.data_ptr(), tk.data_ptr()
    t_sim = timed(lambda: _capi.check(lib.avexhip_retrieval_batch(C.byref(r), s), "retrieval_batch"), reps)
    flops = 2.0 * n * nq * d
    return {"product_rows": nq, "flops": flops, "assign_stage": t_assign, "retr_sim_stage1": t_sim,
            "assign_over_retr_sim": t_assign["median_s"] / t_sim["median_s"],
            "assign_share_of_fp32_mfma_peak": flops / t_assign["median_s"] / PEAK_F32_MFMA,
            "retr_sim_share_of_fp32_mfma_peak": flops / t_sim["median_s"] / PEAK_F32_MFMA}


def one_at_a_time(x, k):
    prep = K._Prepared(x, k, 1, 1e-4)
    rs = np.random.RandomState(42)
    best = None
    for _ in range(10):
        run = K._run(prep, k, 300, rs, None)
        run.pop("_summary")
        inertia = float(run["inertias"][0])
        best = inertia if best is None or inertia < best else best
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--ks", default="64,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=16384)
    ap.add_argument("--cpu-k", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for k in [int(s) for s in a.ks.split(",") if s]:
        x, lab = make(a.n, a.dim, k)
        res = {}
        total = timed(lambda: res.update(K.eval_clustering(x, lab)), a.reps)
        split = {}
        km = K.kmeans(x, k, _timing=split)
        row = {"n": a.n, "d": a.dim, "k": k, "n_init": 10, "eval_clustering": total, "stages_of_one_kmeans_call": split,
               "n_iters": km["n_iters"].tolist(), "best_init": km["best_init"], "inertia": km["inertia"], **res}
        row["assign_ab"] = assign_ab(x, k, max(a.reps, 5))
        lock = timed(lambda: K.kmeans(x, k), a.reps)
        single = timed(lambda: one_at_a_time(x, k), a.reps)
        row["lock_step_kmeans"], row["one_restart_at_a_time_kmeans"] = lock, single
        row["one_at_a_time_over_lock_step"] = single["median_s"] / lock["median_s"]
        row["one_at_a_time_best_inertia_equals_lock_step"] = one_at_a_time(x, k) == km["inertia"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, lab
        torch.cuda.empty_cache()
    cpu = None
    if a.cpu_n > 0:
        x, lab = make(a.cpu_n, a.dim, a.cpu_k)
        dev = timed(lambda: K.eval_clustering(x, lab), a.reps)
        cpu = {"n": a.cpu_n, "d": a.dim, "k": a.cpu_k, "device_eval_clustering": dev, "device_result": K.eval_clustering(x, lab),
               "cpu_threads": torch.get_num_threads()}
        try:
            from sklearn.cluster import KMeans
            from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score, v_measure_score
            xh, lh = x.cpu().numpy(), lab.cpu().numpy()
            t0 = time.perf_counter()
            pred = KMeans(n_clusters=a.cpu_k, random_state=42, n_init=10, max_iter=300).fit_predict(xh)
            got = {"clustering_ari": float(adjusted_rand_score(lh, pred)), "clustering_nmi": float(normalized_mutual_info_score(lh, pred)),
                   "clustering_v_measure": float(v_measure_score(lh, pred))}
            cpu.update({"sklearn_s": time.perf_counter() - t0, "sklearn_result": got, "sklearn_where": "this machine"})
            cpu["sklearn_over_device"] = cpu["sklearn_s"] / dev["median_s"]
        except ImportError:
            cpu["sklearn_where"] = "not importable on this machine"
        print(json.dumps(cpu), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "sizes": rows, "cpu_leg": cpu}, f, indent=1)


if __name__ == "__main__":
    main()
