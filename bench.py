#!/usr/bin/env python3
"""Headline benchmark: clips/s (10 s @ 16 kHz) embedding extraction, BEATs-base, on N MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 256] [--dtype f16|bf16] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path (wav resident in HBM -> fbank -> BEATs-base encoder ->
mean-pooled 768-d embedding) over one batch of synthetic clips per GPU; with N > 1 the batch is
sharded data-parallel (one process per GPU, launched by torch.distributed.run) and the step ends
with one RCCL all-gather of the pooled [B_local, 768] embeddings.  Weak scaling:
per-GPU batch is fixed, `value` is whole-job clips/s.

A plain run sets up, warms up, times K steps, writes the last step's embeddings if --dump-outputs
is given, and prints ONE JSON line (rank 0) with the driver's contract fields.  --full adds,
after the timed region:
  roofline      dominant kernel (the MFMA GEMM): algorithmic FLOPs / HIP-event time on the launch stream
  parity        live parity of the bench configuration against the reference golden
  cpu_baseline  the CPU oracle (NumPy restatement of the reference, "port") timed on this host
and the other legs below (host-to-device rate, board power, configs C3 / C5; with N > 1 the
clip-order check of the gathered matrix and the blocking all-gather time).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SAMPLES = 160000            # 10 s @ 16 kHz
FLOP_PER_CLIP = 98.7e9      # SURVEY.md §8d (FFN 56.17, QKV/out 28.09, SDPA 9.07, pos-conv 4.69, ...)
PEAK_TFLOPS = 2500.0        # dense bf16/f16 MFMA peak, MI355X_MICROARCH.md
DUMP_MAX_BYTES = 64 << 20   # --dump-outputs budget


def dump_outputs(out, out_dir: str) -> None:
    """--dump-outputs: the timed path's last result, as its caller receives it (fp32), so that two builds can be compared output for
    output on identical inputs.  Rows beyond the budget are dropped by a fixed seeded sample (same rows for the same arguments)."""
    import numpy as np
    a = out.detach().float().cpu().numpy()
    if a.nbytes > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // (a.itemsize * a.shape[1])
        a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "pooled.npy"), np.ascontiguousarray(a))


def cpu_baseline_worker(seconds_budget: float) -> None:
    """One worker of the CPU baseline (a fresh process started by cpu_baseline; never touches the GPU): the oracle on one clip at a
    time for `seconds_budget` seconds, BLAS threads as the environment says; prints {"clips", "seconds"}."""
    from avex_amd import synth
    from oracle import beats_oracle as O
    cfg = synth.BEATS_BASE_CFG
    sd = synth.beats_state_dict(cfg, seed=0)
    x = synth.noise_clips(2, SAMPLES, seed=0)
    O.beats_forward(x[:1], sd, cfg)                      # warm-up (BLAS threads, page-in)
    t0 = time.time()
    done = 0
    while True:
        f, _ = O.beats_forward(x[done % 2: done % 2 + 1], sd, cfg)
        O.pooled(f)
        done += 1
        el = time.time() - t0
        if el > seconds_budget or done >= 256:
            break
    print(json.dumps({"clips": done, "seconds": el}), flush=True)


def cpu_baseline(sd, cfg, seconds_budget=20.0):
    """Time the oracle (checker, never shipped) on a bounded sample of the same workload, the way a CPU job would run it: clips are
    independent, so W worker processes of 4 BLAS threads each embed clips side by side (one OpenBLAS pool over all cores spends most of
    its time synchronising on 496-row products: 1.4 clips/s on 32 threads in round 3, below the reference's own 2.6 on 8).  The workers
    are fresh processes (this one has initialised the GPU and must not fork)."""
    import subprocess
    cores = os.cpu_count() or 1
    per = 4 if cores >= 8 else max(1, cores // 2)
    workers = max(1, min(cores // per, 16))
    env = dict(os.environ, OPENBLAS_NUM_THREADS=str(per), OMP_NUM_THREADS=str(per), MKL_NUM_THREADS=str(per))
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", str(seconds_budget)]
    t0 = time.time()
    procs = [subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for _ in range(workers)]
    rate, clips, secs = 0.0, 0, 0.0
    for p in procs:
        try:
            out, _ = p.communicate(timeout=seconds_budget * 4 + 120)
            j = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            rate += j["clips"] / j["seconds"]
            clips += j["clips"]
            secs = max(secs, j["seconds"])
        except Exception:  # noqa: BLE001
            p.kill()
    fixture = None
    try:        # the real reference (PyTorch fp32) timed once in the development container when the goldens were made: a fixture, not this host
        j = json.load(open(os.path.join(ROOT, "tests", "golden", "base_api.json")))
        fixture = {"value": round(4 / j["cpu_reference_seconds"]["b4"], 3), "unit": "clips/s", "kind": "reference",
                   "host": j.get("cpu_reference_host"), "sample": "4 clips x 10 s, avex BEATs forward, recorded by tests/golden/make_goldens.py"}
    except Exception:  # noqa: BLE001
        pass
    return {"value": round(rate, 3), "unit": "clips/s", "cores": workers * per, "kind": "port",
            "sample": f"{clips} clips x 10 s through oracle/beats_oracle.py (NumPy fp32) in {workers} worker processes x {per} OpenBLAS threads, "
                      f"{secs:.1f} s each ({time.time() - t0:.0f} s wall with start-up); host has {cores} logical cores",
            "reference_fixture": fixture}


def board_power(step, sync, device_index: int = 0, seconds: float = 3.0):
    """Outside the timed region, rank 0, one GPU: loop the same step for a few seconds while a thread reads the board's hwmon files
    (power1_input, power1_cap, freq1_input = sclk) straight from sysfs.  The line then says by itself whether the step ran at the power
    cap -- where only joules per clip, not idle cycles, are left to win.  No child process is started (a process
    that has initialised the GPU must not fork-and-exec on this pool, least of all under a profiler).  None if the files are not
    there; never raises."""
    import glob
    import threading
    try:
        import torch
        pr = torch.cuda.get_device_properties(device_index)
        cands = []
        try:
            bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            cands = glob.glob(f"/sys/bus/pci/devices/{bdf}/hwmon/hwmon*")
        except Exception:  # noqa: BLE001
            cands = []
        by_bdf = bool(cands)
        if not cands:
            cands = [d for d in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*") if os.path.exists(os.path.join(d, "power1_input"))]
        if not cands:
            return None

        def rd(path):
            try:
                with open(path) as f:
                    return float(f.read().strip())
            except Exception:  # noqa: BLE001
                return None

        samples, stop = {d: [] for d in cands}, threading.Event()

        def sampler():
            while not stop.is_set():
                for d in cands:
                    pw, ck = rd(os.path.join(d, "power1_input")), rd(os.path.join(d, "freq1_input"))
                    if pw is not None and ck is not None:
                        samples[d].append((pw * 1e-6, ck * 1e-6))
                time.sleep(0.1)

        th = threading.Thread(target=sampler, daemon=True)
        th.start()
        t0 = time.time()
        n = 0
        while time.time() - t0 < seconds:
            step()
            n += 1
            if n % 4 == 0:
                sync()
        sync()
        stop.set()
        th.join(timeout=3)
        med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
        best = max((d for d in cands if len(samples[d]) >= 3), key=lambda d: med([p for p, _ in samples[d]]), default=None)
        if best is None:
            return None
        pw = [p for p, _ in samples[best]]
        ck = [c for _, c in samples[best]]
        cap = rd(os.path.join(best, "power1_cap"))
        return {"median_w": round(med(pw), 1), "max_w": round(max(pw), 1), "cap_w": round(cap * 1e-6, 1) if cap else None,
                "sclk_median_mhz": round(med(ck)), "sclk_peak_mhz": 2400, "samples": len(pw),
                "how": f"sysfs hwmon (power1_input, freq1_input) every 0.1 s while the same step loops for {seconds:.0f} s after the timed region"
                       + ("" if by_bdf else "; device picked as the busiest hwmon on the node")}
    except Exception:  # noqa: BLE001
        return None


DTYPE_NOTE = ("BASELINE.json's config says bf16; the MFMA operands here are f16 (same width, same 2.5 PFLOP/s dense rate on gfx950): bf16's 8-bit "
              "mantissa on the WEIGHTS alone puts the pooled embedding at 2e-3 of the fp32 reference, outside north_star's 1e-3; f16 is at 3e-4 "
              "(both measured live in `parity`).  Accumulation, residual sums, LayerNorm, softmax statistics and the frontend are fp32; --dtype bf16 "
              "runs the bf16 path")


def parity_vs_golden(cfg, sd, args, enc, wav):
    """Outside the timed region: the four clips of tests/golden/base_api.npz:b4 (outputs of the real reference, fp32 CPU) take rows 0-3 of
    the bench's own batch and go through the bench's own configuration, for both operand types.  The launches have the benchmark's
    shapes (so a profiler's per-kernel averages of the same command are not diluted by small launches; the bf16 instantiations show
    up under their own kernel names)."""
    import numpy as np
    import torch
    from avex_amd import kernels as K
    from avex_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "base_api.npz"))["b4.pooled"]
    x = wav.clone()
    n = min(4, x.shape[0])
    x[:n] = torch.from_numpy(synth.noise_clips(4, SAMPLES, seed=0)[:n]).to(x.device)
    out = {"reference": "tests/golden/base_api.npz:b4.pooled (avex BEATs, fp32 CPU, same synthetic checkpoint)", "tolerance": 1e-3,
           "how": f"the golden's clips at rows 0..{n - 1} of the {x.shape[0]}-clip bench batch"}
    for dt in ("f16", "bf16"):
        e = enc if dt == args.dtype else K.BeatsEncoder(cfg, sd, operand_dtype=dt, max_chunk_clips=args.chunk, residual=args.residual)
        p = e.forward(x, want_features=False, want_pooled=True)["pooled"][:n].cpu().numpy()
        if e is not enc:
            e.close()
        out[f"pooled_rel_l2_{dt}"] = float(f"{np.linalg.norm(p - g[:n]) / np.linalg.norm(g[:n]):.3e}")
    return out


def effnet_algorithmic_bytes(stages, H, W, samples, stem=32, head=1280):
    """EfficientNet on one clip, layer by layer: every convolution reads its input once and writes its output once in the operand type
    (2 bytes), at the REAL channel counts; the mel frontend reads the fp32 wav and writes the fp32 image; weights (4 M parameters, L2-
    resident) are not counted.  No cross-layer fusion is assumed -- it is the traffic of the algorithm as the reference structures it
    (efficientnet.py:163-215: torchvision's features stack), the figure SURVEY.md section 8d asks the C5 rate to be priced with."""
    co = lambda n, k, s: (n + 2 * ((k - 1) // 2) - k) // s + 1      # noqa: E731
    b = samples * 4 + H * W * 4 + H * W * 4                         # frontend in / out, stem in
    H, W = co(H, 3, 2), co(W, 3, 2)
    b += H * W * stem * 2
    c = stem
    for er, k, s, cin, cout, reps in stages:
        for r in range(reps):
            st, ci = (s if r == 0 else 1), (cin if r == 0 else cout)
            ce = ci * er
            if er != 1:
                b += H * W * (ci + ce) * 2                          # expand 1x1
            Ho, Wo = co(H, k, st), co(W, k, st)
            b += (H * W + Ho * Wo) * ce * 2                         # depthwise (the squeeze pool rides on its way out)
            b += Ho * Wo * (ce + cout) * 2                          # squeeze-scaled projection 1x1
            if st == 1 and ci == cout:
                b += Ho * Wo * cout * 2                             # residual
            H, W, c = Ho, Wo, cout
    return b + H * W * (c + 2 * head) * 2 + head * 4                # head 1x1 (in, out), global pool (in, out)


def other_configs(steps: int = 5):
    """BASELINE.json configs C3 (EAT, 512 x 5 s) and C5 (EfficientNet-B0, 1024 x 10 s) after the headline's timed region, same box, same
    process: ms per step, clips/s, a roofline each, and the pooled embedding of two clips against tests/golden/family_small.npz -- outputs
    of the NumPy oracles on the synthetic checkpoints (tests/golden/make_family_goldens.py).  PARITY UNPINNED for both families: the
    arithmetic they restate is third-party code absent from the reference tree, so those vectors pin the HIP
    path to the oracle, not to the reference.  Not the headline `value`."""
    import numpy as np
    import torch
    from avex_amd import kernels as K
    from avex_amd import synth
    from avex_amd.eat_encoder import EatEncoder
    from avex_amd.effnet_encoder import EfficientNetB0Encoder
    gold = np.load(os.path.join(ROOT, "tests", "golden", "family_small.npz"))
    rel = lambda a, b: float(f"{np.linalg.norm(a - b) / np.linalg.norm(b):.3e}")      # noqa: E731
    out = {}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    try:        # ---- C3: EAT-base (eat_hf.py:241-289), 512 clips x 5 s -> mean over the 513 tokens
        B, n = 512, 80000
        enc = EatEncoder(synth.EAT_BASE_CFG, synth.eat_state_dict(), operand_dtype="f16")
        wav = torch.from_numpy(synth.noise_clips(B, n, seed=0)).cuda()
        dt = timed(lambda: enc.forward(wav, want_features=False, pooling="mean")["pooled"])
        fl = 2 * 512 * 256 * 768 + 12 * (2 * 513 * 768 * (2304 + 768 + 3072 + 3072) + 4 * 513 * 513 * 768)      # per clip: patch GEMM + 12 blocks
        small = torch.from_numpy(synth.noise_clips(2, n, seed=int(gold["eat.seed"][0]))).cuda()
        p = enc.forward(small, want_features=False, pooling="mean")["pooled"].cpu().numpy()
        out["c3_eat"] = {"workload": "EAT-base (12L/768/3072/12H, 513 tokens), batch 512 x 5 s @ 16 kHz, wav resident in HBM -> mean-pooled 768-d",
                         "ms_per_step": round(1e3 * dt, 3), "clips_per_s": round(B / dt, 1), "dtype": "f16",
                         "roofline": {"bound": "mfma", "achieved": round(B * fl / dt / 1e12, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                                      "frac": round(B * fl / dt / 1e12 / PEAK_TFLOPS, 4), "gflop_per_clip": round(fl / 1e9, 2)},
                         "parity": {"reference": "tests/golden/family_small.npz:eat.pooled_mean (oracle/eat_oracle.py, UNPINNED: EAT's remote code is absent from the reference tree)",
                                    "how": "2 clips x 5 s; the token mean on the operand-type residual stream (the timed path), the class token -- the reference wrapper's "
                                           "default pooling, eat_hf.py:149,281-282 -- on the fp32 stream EatEncoder(residual='auto') takes for un-averaged rows",
                                    "pooled_rel_l2_f16": rel(p, gold["eat.pooled_mean"]),
                                    "cls_token_rel_l2_f16": rel(enc.forward(small, want_features=False, pooling="cls")["pooled"].cpu().numpy(), gold["eat.cls"]),
                                    "tolerance": 1e-3}}
        enc.close()
        del wav, enc
    except Exception as e:  # noqa: BLE001
        out["c3_eat"] = {"error": repr(e)[:300]}
    try:        # ---- C5: EfficientNet-B0 (efficientnet.py:163-215), 1024 clips x 10 s -> mel 128 x 1001 -> features -> global average pool
        B, n = 1024, 160000
        enc = EfficientNetB0Encoder(synth.effnet_b0_state_dict())
        plan = K.MelspecPlan(n_fft=800, hop_length=160, n_mels=128, normalize=True)
        wav = torch.from_numpy(synth.noise_clips(B, n, seed=0)).cuda()      # the build's counter-based generator, as the C3 leg and the headline
        dt = timed(lambda: enc.forward(plan(wav), want_features=False, want_pooled=True)["pooled"])
        nbytes = effnet_algorithmic_bytes(synth.EFFNET_B0_STAGES, 128, 1 + n // 160, n)
        counted = None      # HBM-side bytes per clip from the committed PMC passes of the same forward (scripts/pmc_effnet.sh), not measured in this run
        try:
            import glob
            cf = sorted(glob.glob(os.path.join(ROOT, "profiles", "r??_effnet_traffic.json")))
            cj = json.load(open(cf[-1]))
            counted = {"mb_per_clip": cj["counted_mb_per_clip"], "mb_per_clip_fetch_undoubled": cj["counted_mb_per_clip_fetch_undoubled"],
                       "over_algorithmic": cj["counted_over_algorithmic"], "source": "profiles/" + os.path.basename(cf[-1]), "measured_in_this_run": False,
                       "note": "FETCH_SIZE doubled (the gfx950 rule for wide coalesced reads: an upper bound for the narrower depthwise / squeeze reads) + WRITE_SIZE; "
                               "below the algorithmic figure because the fused block fronts never write the 6 x expanded tensors"}
        except Exception:  # noqa: BLE001
            counted = None
        small = torch.from_numpy(synth.noise_clips(2, n, seed=int(gold["effnet.seed"][0]))).cuda()
        p = enc.forward(plan(small), want_features=False, want_pooled=True)["pooled"].cpu().numpy()
        out["c5_effnet"] = {"workload": "EfficientNet-B0 (torchvision features stack, BatchNorm folded), batch 1024 x 10 s @ 16 kHz, wav resident in HBM -> "
                                        "mel 128 x 1001 -> pooled 1280-d; expansion + depthwise + squeeze sums of the narrow-input blocks in one HIP kernel, depthwise through LDS, the other 1x1 convolutions on the MFMA GEMMs",
                            "ms_per_step": round(1e3 * dt, 3), "clips_per_s": round(B / dt, 1), "dtype": "f16",
                            "roofline": {"bound": "hbm", "achieved": round(B * nbytes / dt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                                         "frac": round(B * nbytes / dt / 1e9 / 8000.0, 4), "algorithmic_mb_per_clip": round(nbytes / 1e6, 2),
                                         "traffic": counted,
                                         "achieved_counted": (round(B * counted["mb_per_clip"] * 1e6 / dt / 1e9, 1) if counted else None),
                                         "frac_counted": (round(B * counted["mb_per_clip"] * 1e6 / dt / 1e9 / 8000.0, 4) if counted else None),
                                         "how": "every layer's input read once + output written once at 2 bytes and the real channel counts, no fusion assumed (bench.py effnet_algorithmic_bytes)"},
                            "parity": {"reference": "tests/golden/family_small.npz:effnet.pooled (oracle/effnet_oracle.py, UNPINNED: torchvision is absent from the reference tree)",
                                       "how": "2 clips x 10 s", "pooled_rel_l2_f16": rel(p, gold["effnet.pooled"]), "tolerance": 1e-3}}
        del wav, enc
    except Exception as e:  # noqa: BLE001
        out["c5_effnet"] = {"error": repr(e)[:300]}
    torch.cuda.empty_cache()
    return out


def h2d_inclusive(enc, wav, steps: int):
    """Outside the timed region, N = 1: the same step when the caller hands over HOST buffers (fp32 wav, 640 KB per clip: SURVEY.md
    section 8d asks for this second number).  The batch sits in pinned host memory; batch n + 1 crosses PCIe on a copy stream while
    batch n runs (what avex_amd.extraction does), so `steps` timed steps are `steps` host-to-device copies + `steps` forwards.
    Never the headline `value`."""
    import torch
    try:
        B = wav.shape[0]
        pinned = torch.empty(wav.shape, dtype=wav.dtype, pin_memory=True)
        pinned.copy_(wav)
        side = torch.cuda.Stream()
        main = torch.cuda.current_stream()

        def run(n):
            with torch.cuda.stream(side):
                cur = pinned.to(wav.device, non_blocking=True)
                ev = torch.cuda.Event(); ev.record(side)
            main.wait_event(ev)
            out = None
            for i in range(n):
                nxt, ev = None, None
                if i + 1 < n:
                    with torch.cuda.stream(side):
                        nxt = pinned.to(wav.device, non_blocking=True)
                        ev = torch.cuda.Event(); ev.record(side)
                cur.record_stream(main)
                out = enc.forward(cur, want_features=False, want_pooled=True)["pooled"]
                if ev is not None:
                    main.wait_event(ev)
                cur = nxt
            return out

        run(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return {"value": round(B * steps / dt, 2), "unit": "clips/s", "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps,
                "bytes_per_step": int(wav.numel() * 4),
                "how": "fp32 wav in pinned host memory, batch n+1 copied on a side stream while batch n runs (the first copy is inside the timed "
                       "region); not the headline value, which has the wav resident in HBM"}
    except Exception as e:  # noqa: BLE001
        return {"value": None, "error": str(e)[:200]}


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` from a plain shell: start the N ranks as a CHILD `torch.distributed.run` (one process per GPU) and
    relay its output and exit code.  This parent has not imported torch or made any HIP call (a process that has initialised the
    GPU must not be replaced by, or fork into, GPU work on this pool), and it does not exec."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on these hosts (RCCL across processes)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env.setdefault("NCCL_DEBUG", "WARN")                    # RCCL warnings on stderr; on failure the tail is printed below
    import collections
    import threading
    tail = collections.deque(maxlen=80)

    def pump():      # stderr passes through live AND its tail is kept for the failure report
        for ln in proc.stderr:
            sys.stderr.write(ln)
            tail.append(ln)

    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    th = threading.Thread(target=pump, daemon=True)
    th.start()
    for ln in proc.stdout:           # rank 0's single JSON line (and nothing else on stdout) passes through unchanged
        sys.stdout.write(ln)
        sys.stdout.flush()
    rc = proc.wait()
    th.join(timeout=5)
    if rc != 0:
        sys.stderr.write(f"[bench launcher] {n} ranks exited with code {rc}; last lines of their stderr (NCCL_DEBUG={env.get('NCCL_DEBUG')}, "
                         f"HSA_ENABLE_IPC_MODE_LEGACY={env.get('HSA_ENABLE_IPC_MODE_LEGACY')}, master 127.0.0.1:{port}):\n" + "".join(tail))
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256, help="clips per GPU per step")
    ap.add_argument("--dtype", default=os.environ.get("AVEX_AMD_OPERAND", "f16"))
    ap.add_argument("--chunk", type=int, default=int(os.environ.get("AVEX_AMD_CHUNK", "256")))
    ap.add_argument("--residual", default=os.environ.get("AVEX_AMD_RESIDUAL", "half"), choices=["f32", "half"],
                    help="inter-kernel residual stream: fp32, or the operand type (default; pooled parity unchanged)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (rank 0: the pooled [N*B, 768] fp32 embeddings in clip order) "
                         f"to DIR/pooled.npy; above {DUMP_MAX_BYTES >> 20} MB a fixed seeded sample of its rows, in row order")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also measure and check everything beyond the headline: roofline and per-kernel bounds, live "
                         "parity, host-to-device rate, board power, configs C3 / C5, the CPU baseline; with N > 1 the gathered-matrix checks")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-power", action="store_true", help="with --full: skip the post-run board power / clock sample (sysfs hwmon)")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip BASELINE configs C3 (EAT) and C5 (EfficientNet-B0) after the timed region")
    ap.add_argument("--cpu-dry-run", action="store_true",
                    help="tests only: run the launch / barrier / timing / all-gather / JSON control flow on the CPU with gloo and a stub "
                         "in place of the encoder (no number it prints is a measurement)")
    ap.add_argument("--cpu-baseline-worker", type=float, default=0.0, help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.cpu_baseline_worker > 0:
        cpu_baseline_worker(args.cpu_baseline_worker)      # a worker of the cpu_baseline leg: NumPy only, no torch, no GPU
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))      # plain `python bench.py --gpus N`: this parent never touches the GPU

    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        print(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}", file=sys.stderr)
        sys.exit(2)
    dry = args.cpu_dry_run
    if not dry and not torch.cuda.is_available():
        print("bench.py needs a GPU (no CPU fallback for the product path)", file=sys.stderr)
        sys.exit(2)
    if dry:
        dev = torch.device("cpu")
        sync = lambda: None
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        sync = torch.cuda.synchronize
    if world > 1:
        import datetime
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("NCCL_DEBUG", "WARN")                   # RCCL's warnings go to stderr: the launcher keeps the tail of every rank's
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on these hosts
        timeout = datetime.timedelta(seconds=int(os.environ.get("AVEX_AMD_DIST_TIMEOUT_S", "300")))
        try:
            if dry:
                dist.init_process_group(backend="gloo", timeout=timeout)
            else:
                dist.init_process_group(backend="nccl", device_id=dev, timeout=timeout)
            dist.barrier()                                            # the first collective: communicator set-up (xGMI rings) happens here
        except Exception as e:  # noqa: BLE001
            print(f"[bench rank {rank}/{world} local {local_rank}] rendezvous / first collective FAILED after <= {timeout.seconds} s: {e!r}; "
                  f"MASTER_ADDR={os.environ.get('MASTER_ADDR')} MASTER_PORT={os.environ.get('MASTER_PORT')} "
                  f"HSA_ENABLE_IPC_MODE_LEGACY={os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')} backend={'gloo' if dry else 'nccl'} "
                  f"visible devices={torch.cuda.device_count() if not dry else 'cpu'}", file=sys.stderr, flush=True)
            sys.exit(3)

    from avex_amd import build, synth
    cfg = synth.BEATS_BASE_CFG
    if dry:
        class _Stub:      # stands in for the encoder in the CPU dry run: per-clip function of the input, [B, 768]
            def forward(self, wav, want_features=False, want_pooled=True):
                return {"pooled": wav[:, :768].contiguous() * 2.0}
        enc, sd = _Stub(), None
    else:
        from avex_amd import kernels as K
        # the library is prebuilt in tree; if it is stale only rank 0 compiles, the others wait for it
        if rank == 0:
            build.build(verbose=False)
        if world > 1:
            dist.barrier()
        sd = synth.beats_state_dict(cfg, seed=0)
        enc = K.BeatsEncoder(cfg, sd, operand_dtype=args.dtype, max_chunk_clips=args.chunk, residual=args.residual)

    B = args.batch
    # synthetic clips keyed by GLOBAL clip index: rank r owns clips [r*B, (r+1)*B) of one seed-0 stream of
    # 0.1 * N(0,1) clips from the build's own counter-based PRNG, so any sharding of the job embeds the same clips
    wav = torch.from_numpy(synth.noise_clips(B, SAMPLES, seed=0, first_clip=rank * B)).to(dev)
    gathered = torch.empty((world * B, 768), dtype=torch.float32, device=dev) if world > 1 else None
    # N > 1: the step's all-gather is NON-BLOCKING (avex_amd.dist.PipelinedGather): the gather of step n runs on the communicator's
    # stream under the kernels of step n + 1 and is waited for one step later; the last one is flushed inside the timed region, so
    # K steps are K forwards + K completed gathers ("overlap gather(n) with compute(n+1)")
    from avex_amd.dist import PipelinedGather
    pipe = PipelinedGather(measure=True) if world > 1 else None

    def step():
        r = enc.forward(wav, want_features=False, want_pooled=True)
        if pipe is not None:
            return pipe.push(r["pooled"], world * B)        # the PREVIOUS step's gathered matrix (None at the first step)
        return r["pooled"]

    out = None
    for _ in range(args.warmup):
        out = step()
    if pipe is not None:
        out = pipe.flush()
        pipe.exposed_ms()            # (reset: the warm-up's waits are not the timed region's)
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    if pipe is not None:
        out = pipe.flush()
    sync()
    own_elapsed = time.perf_counter() - t0      # this rank's K steps + K completed gathers, before it waits for the others
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    per_rank = None
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # per-rank view, so that a slow first 8-GPU run says WHERE it is slow: each rank's own time for the K steps and the time its
        # compute stream spent waiting for gathers that had not finished under the next step's kernels
        mine = torch.tensor([own_elapsed, pipe.exposed_ms() / 1e3], dtype=torch.float64, device=dev)
        allr = torch.empty((world * 2,), dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(allr, mine)
        allr = allr.cpu().reshape(world, 2)
        ms = (allr[:, 0] * 1e3 / args.steps).tolist()
        ex = (allr[:, 1] * 1e3 / args.steps).tolist()
        per_rank = {"ms_per_step_min": round(min(ms), 3), "ms_per_step_max": round(max(ms), 3), "slowest_rank": int(max(range(world), key=lambda r: ms[r])),
                    "ms_per_step": [round(v, 3) for v in ms],
                    "exposed_gather_ms_per_step_max": round(max(ex), 4), "exposed_gather_ms_per_step_mean": round(sum(ex) / world, 4)}
    assert torch.isfinite(out).all()
    if rank == 0 and args.dump_outputs:
        dump_outputs(out, args.dump_outputs)

    # ---- after the timed region (--full): the gathered matrix is in clip order on every rank ----
    gather_check = None
    all_gather_ms = None
    if world > 1 and args.full:
        local = enc.forward(wav, want_features=False, want_pooled=True)["pooled"]
        dist.all_gather_into_tensor(gathered, local)
        piped_ok = torch.equal(out, gathered)                                      # what the timed loop's last (pipelined) gather delivered
        # the exchange alone, blocking form, event-timed on the compute stream (rank 0's view; 10 repetitions)
        sync()
        if dry:
            tg = time.perf_counter()
            for _ in range(10):
                dist.all_gather_into_tensor(gathered, local)
            all_gather_ms = (time.perf_counter() - tg) * 1e3 / 10
        else:
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            for _ in range(10):
                dist.all_gather_into_tensor(gathered, local)
            g1.record()
            sync()
            all_gather_ms = g0.elapsed_time(g1) / 10
        ok_own = torch.equal(gathered[rank * B:(rank + 1) * B], local)            # my rows sit at my clip indices, bit for bit
        sums = torch.empty((world * B,), dtype=torch.float64, device=dev)          # a checksum of checksums: every rank's
        dist.all_gather_into_tensor(sums, local.double().sum(1).contiguous())      # per-clip sums, gathered separately,
        ok_all = torch.equal(sums, gathered.double().sum(1))                       # must match the gathered rows
        flag = torch.tensor([1 if (ok_own and ok_all and piped_ok) else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        gather_check = bool(flag.item())
        if dry:     # the stub is a closed form of the clip, so the whole matrix can be checked against the generator
            want = torch.from_numpy(synth.noise_clips(world * B, SAMPLES, seed=0)[:, :768].copy()) * 2.0
            gather_check = gather_check and torch.equal(gathered.cpu(), want)
        assert gather_check, "all-gathered embeddings are not in clip order"

    # ---- roofline of the dominant kernel (rank 0): HIP events around every launch, same stream ----
    roof = None
    stages = None
    others = None
    if rank == 0 and not dry and args.full:
        enc.set_profiling(True)
        enc.forward(wav, want_features=False, want_pooled=True)
        prof = enc.last_profile()
        enc.set_profiling(False)
        # the dominant kernel: the four GEMMs of every encoder layer (QKV, out_proj, fc1, fc2), all in the streaming 256-tile kernel
        # gemm256p_kernel (with the default fold its instantiations <T, 1, 1> / <T, 2, 3> carry the encoder's LayerNorms too)
        layer_gemms = ("gemm.qkv", "gemm.out_proj", "gemm.fc1", "gemm.fc2")
        gemm_ms = sum(ms for n, ms, fl in prof if n in layer_gemms)
        gemm_fl = sum(fl for n, ms, fl in prof if n in layer_gemms)
        n_streams = max(1, min(4, int(os.environ.get("AVEX_AMD_STREAMS", "1") or 1)))       # (a knob, default 1: api.cpp plan_chunks)
        eff_chunk = args.chunk if n_streams == 1 or B < 2 else min(args.chunk, (B + n_streams - 1) // n_streams)
        n_gemm_launch = 4 * int(cfg["encoder_layers"]) * ((B + eff_chunk - 1) // eff_chunk)
        kernel_name = "gemm256p_kernel"
        ln_fold = args.residual == "half" and os.environ.get("AVEX_AMD_LN_FOLD", "1") not in ("0",)
        total_ms = sum(ms for _, ms, _ in prof)
        stages = {n: {"ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1) if ms > 0 and fl > 0 else None} for n, ms, fl in prof}
        # the other kernels of the step against their own bounds (same serialised HIP-event times; algorithmic bytes / flops of DESIGN.md section 4)
        sm = {n: ms for n, ms, _ in prof}
        sf = {n: fl for n, ms, fl in prof}
        L, T_, E_ = int(cfg["encoder_layers"]), 496, 768
        others = {}
        if sm.get("attention"):
            att_name = "attention2_kernel" if os.environ.get("AVEX_AMD_ATT_VARIANT", "3") == "2" else "attention3_kernel"      # (up to 512 tokens; attention.hip's launcher)
            others[att_name] = {"bound": "mfma", "achieved": round(sf["attention"] / sm["attention"] / 1e9, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                                           "frac": round(sf["attention"] / sm["attention"] / 1e9 / PEAK_TFLOPS, 4), "ms_per_step": round(sm["attention"], 3)}
        if sm.get("posconv"):
            others["posconv_kernel"] = {"bound": "mfma", "achieved": round(sf["posconv"] / sm["posconv"] / 1e9, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                                        "frac": round(sf["posconv"] / sm["posconv"] / 1e9 / PEAK_TFLOPS, 4), "ms_per_step": round(sm["posconv"], 3)}
        if sm.get("layernorm") and args.residual == "half":
            # patch LayerNorm (half -> half, 512 wide) and encoder LayerNorm (half -> half, 768 wide); without the fold also 2 per layer
            ln_bytes = B * T_ * 512 * 2 * 2 + B * T_ * E_ * 2 * 2 + (0 if ln_fold else (2 * L - 1) * B * T_ * E_ * 2 * 2)
            others["layernorm_half_kernel"] = {"bound": "hbm", "achieved": round(ln_bytes / sm["layernorm"] / 1e9, 2), "peak": 8.0, "unit": "TB/s",
                                               "frac": round(ln_bytes / sm["layernorm"] / 1e9 / 8.0, 4), "ms_per_step": round(sm["layernorm"], 3),
                                               "launches_per_step": 2 if ln_fold else 2 * L + 1,
                                               "note": "read + write mix; torch's device-to-device copy reaches 5.3 TB/s on this board (scripts/hbm_bw.py)"
                                                       + ("; the encoder's 24 LayerNorms are folded into the GEMM epilogues" if ln_fold else "")}
        if sm.get("fbank"):
            fb_bytes = B * (SAMPLES * 4 + 992 * 128 * 2)
            others["fbank_kernel"] = {"bound": "hbm", "achieved": round(fb_bytes / sm["fbank"] / 1e9, 2), "peak": 8.0, "unit": "TB/s",
                                      "frac": round(fb_bytes / sm["fbank"] / 1e9 / 8.0, 4), "ms_per_step": round(sm["fbank"], 3),
                                      "note": "vector-instruction-bound (898 W, full clock): profiles/r02f_fbank_stages.txt"}
        ach = gemm_fl / (gemm_ms * 1e-3) / 1e12
        traffic = None     # HBM bytes per GEMM launch from the committed rocprofv3 PMC passes (scripts/collect_profiles.sh)
        import glob
        tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r??_traffic.json")))      # the latest round's PMC summary
        traffic_src = None
        traffic_by_shape = None
        if tfiles and B == 256 and args.dtype == "f16":
            try:
                tj = json.load(open(tfiles[-1]))
                loop = tj.get("gemm256p_kernel_layer_loop")       # the 48 layer GEMMs only (scripts/parse_traffic.py labels launches by position)
                traffic = round((loop or tj[kernel_name])["hbm_bytes_per_launch"])
                traffic_src = "profiles/" + os.path.basename(tfiles[-1])
                alg = {"qkv": B * T_ * (E_ + 3 * E_) * 2 + 3 * E_ * E_ * 2, "out_proj": B * T_ * (E_ + 2 * E_) * 2 + E_ * E_ * 2,
                       "fc1": B * T_ * (E_ + 4 * E_) * 2 + 4 * E_ * E_ * 2, "fc2": B * T_ * (4 * E_ + 2 * E_) * 2 + 4 * E_ * E_ * 2}
                if tj.get("gemm256p_kernel_by_shape"):
                    traffic_by_shape = {k: {"counted": round(v["hbm_bytes_per_launch"]), "algorithmic": alg.get(k)}
                                        for k, v in tj["gemm256p_kernel_by_shape"].items() if k in alg}
            except Exception:  # noqa: BLE001
                traffic = None
        # rocprof-reported MFMA utilisation of the same kernel (north_star): SQ counters, one --pmc pass set per GEMM shape
        # (scripts/pmc_gemm_sq.sh -> profiles/rNN_gemm_sq.json): "frac of the 2.4 GHz peak" = clock held / 2400 x matrix-pipe busy share x issue efficiency
        sq = {}
        sfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r??_gemm_sq.json")))
        if sfiles:
            try:
                sj = json.load(open(sfiles[-1]))
                tw = sj["layer_gemms_time_weighted"]
                # do these counters describe the kernel this run executes?  (the summary records the hash of gemm.hip + common.h it was collected on)
                from avex_amd.build import kernel_source_sha16
                here = kernel_source_sha16(("gemm.hip", "gemm_epi.h", "common.h"))
                sq = {"sq_same_kernel_source": sj.get("gemm_source_sha16") == here, "sq_kernel_source_sha16": {"counters": sj.get("gemm_source_sha16"), "this_run": here},
                      "mfma_busy_frac": tw["mfma_busy_frac"], "effective_clock_mhz": tw["effective_clock_mhz"],
                      "mfma_busy_by_shape": {k: {"mfma_busy_frac": v["mfma_busy_frac"], "effective_clock_mhz": v["effective_clock_mhz"]}
                                             for k, v in sj.items() if k in ("qkv", "out", "fc1", "fc2")},
                      "sq_source": "profiles/" + os.path.basename(sfiles[-1]) + " (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES, GRBM_GUI_ACTIVE ...; busy = matrix-pipe busy cycles / "
                                   "(shader cycles x 1024 SIMDs); clock = GRBM_GUI_ACTIVE / 8 / kernel time)"}
            except Exception:  # noqa: BLE001
                sq = {}
        roof = {"bound": "mfma", "kernel": kernel_name, "achieved": round(ach, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src, "traffic_by_shape": traffic_by_shape,
                "measured_in_this_run": {"achieved": True, "avg_launch_ms": True, "traffic": False, "traffic_by_shape": False, "mfma_busy_frac": False,
                                         "effective_clock_mhz": False,
                                         "note": "traffic and the SQ fields are read from the committed rocprofv3 --pmc summaries named in traffic_source / sq_source (same command, "
                                                 "another box: counters cannot be collected inside a timed run)"},
                "algorithmic_tflop_per_launch": round(gemm_fl / n_gemm_launch / 1e12, 4),
                "launches_per_step": n_gemm_launch, "avg_launch_ms": round(gemm_ms / n_gemm_launch, 4),
                "gemm_share_of_step": round(gemm_ms / total_ms, 3), **sq,
                "note": "peak is the 2.4 GHz dense MFMA figure; this kernel (and the step as a whole) runs at the board's 1400 W power cap, "
                        "shader clock 1.5-1.9 GHz on random operands (profiles/r01c_gemm_power.txt, profiles/r01e_step_power.txt); a register-only MFMA loop "
                        "on random halves sustains 1.8 PFLOP/s under that cap, 1.4 with this kernel's LDS traffic (profiles/r01h_mfma_power.txt); "
                        "traffic = bytes per launch from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command (FETCH_SIZE doubled, "
                        "the gfx950 correction), algorithmic bytes per launch 0.88 GB; the counters sit between the L2s and the fabric, so the A panels "
                        "re-fetched by the wide K = 768 products (195 MB, inside the 256 MB Infinity Cache) are counted although they need not reach HBM "
                        "(DESIGN.md section 4, 'What the traffic figure is')"}

    if rank == 0:
        clips = world * B * args.steps
        value = clips / elapsed
        line = {
            "metric": "clips/s (10 s @ 16 kHz) embedding extraction, BEATs-base",
            "value": round(value, 2), "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"BEATs-base (12L/768/3072/12H, 90.7 M params, synthetic weights), batch {B} x 10 s @ 16 kHz per GPU, "
                                   f"wav resident in HBM -> mean-pooled 768-d embedding" + (", RCCL all-gather of pooled embeddings" if world > 1 else ""),
                       "global_batch": world * B, "samples_per_clip": SAMPLES, "tokens_per_clip": 496,
                       "parallelism": f"dp{world}", "world_size": dist.get_world_size() if world > 1 else 1,
                       "backend": (dist.get_backend() if world > 1 else None), "gathered_rows_in_clip_order": gather_check,
                       "all_gather": (None if world == 1 else {"form": "non-blocking, overlapped with the next step's kernels, last one flushed inside the timed region",
                                                               "blocking_ms": None if all_gather_ms is None else round(all_gather_ms, 4), "bytes_per_rank": B * 768 * 4,
                                                               "exposed_ms": per_rank["exposed_gather_ms_per_step_max"],
                                                               "exposed_ms_how": "per step, the slowest rank: time its compute stream waited for a gather that had not finished under the next step's kernels (two events around the stream dependency)"}),
                       "per_rank": per_rank,
                       "inputs": "avex_amd.synth.noise_clips(seed=0), keyed by global clip index",
                       "chunk_clips": args.chunk, "streams": max(1, min(4, int(os.environ.get("AVEX_AMD_STREAMS", "1") or 1))), "residual_stream": args.residual,
                       "layernorm_fold": bool(args.residual == "half" and os.environ.get("AVEX_AMD_LN_FOLD", "1") != "0"),
                       "dtype_note": DTYPE_NOTE,
                       "model_tflops_per_s": round(value * FLOP_PER_CLIP / 1e12, 1),
                       "model_frac_of_mfma_peak": round(value * FLOP_PER_CLIP / 1e12 / (PEAK_TFLOPS * world), 4)},
            "roofline": roof, "other_kernels": others, "stages_ms": stages,
        }
        if dry:
            line["data"] = "cpu dry run (control flow only, not a measurement)"
        if world > 1 and args.full:
            # The first multi-GPU line checked against DESIGN.md section 5's list, on stderr (stdout stays one JSON line): what a reader of
            # SCALE_rNN.json should see before trusting the per-N values.
            c = line["config"]
            spread = (per_rank["ms_per_step_max"] - per_rank["ms_per_step_min"]) / max(per_rank["ms_per_step_min"], 1e-9)
            checks = [("world_size == n_gpus", c["world_size"] == world),
                      ("backend nccl (RCCL)" if not dry else "backend (dry run: gloo)", dry or c["backend"] == "nccl"),
                      ("gathered rows in clip order", c["gathered_rows_in_clip_order"] is True),
                      ("exposed gather <= 0.05 ms per step", c["all_gather"]["exposed_ms"] <= 0.05),
                      ("per-rank step spread <= 12 % (measured board-to-board variance)", spread <= 0.12)]
            bad = [n for n, ok in checks if not ok]
            print(f"[bench] multi-GPU checklist ({world} ranks): " + ("all 5 hold" if not bad else "FAILED: " + "; ".join(bad))
                  + f" (exposed gather {c['all_gather']['exposed_ms']} ms, spread {100 * spread:.1f} %, slowest rank {per_rank['slowest_rank']})", file=sys.stderr, flush=True)
            line["config"]["checklist"] = {n: bool(ok) for n, ok in checks}
        full = world == 1 and not dry and args.full
        if full:
            line["parity"] = parity_vs_golden(cfg, sd, args, enc, wav)
            line["config"]["h2d_included"] = h2d_inclusive(enc, wav, max(args.steps, 5))
        if full and not args.no_power:
            line["power"] = board_power(step, sync, local_rank)
        if full and not args.no_other_configs:
            line["configs"] = other_configs()
        if full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(sd, cfg)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
