#!/usr/bin/env python3
"""Which kernels the GEMM and attention dispatch really launch, from a kernel trace -- the cases of tests/test_dispatch_cpu.py that
kernels.gemm / kernels.attention can express, issued on the device, so that the CPU test's table can be held against a library that has
no planner (the commit before it) and two libraries against each other.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 scripts/dispatch_trace.py      # under AVEX_AMD_LIB=... for another build
    python3 scripts/dispatch_trace.py --check OUT/.../*kernel_trace.csv [--against OTHER_kernel_trace.csv]

--check walks the trace's GEMM / attention dispatches in order and holds kernel name (with template arguments), grid in workgroups,
workgroup size and LDS bytes against the expectation of every case (a profiler that reports only a kernel's static LDS shows 0 for these
kernels, whose LDS is all dynamic: the bytes are then not held against anything); --against also compares the two traces dispatch by dispatch.
Knobs read once per process (AVEX_AMD_GEMM_256_MIN_TILES, _NT) and AVEX_AMD_GEMM_VARIANT (read once per process before the planner)
are not switched here; post_ln_* is reached through a one-clip BEATs forward."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S5, T128 = (512, 163840), (256, 65536)
F16 = "_Float16"


def stream(epi, ln, act, grid):
    return (f"gemm256p_kernel<{F16},{epi},{ln},{act}>", (grid, 1)) + S5


def tile128(grid, S=1, reg=False):
    return (f"gemm_nt_kernel<{F16},{'false' if reg else 'true'}>", (grid, S)) + T128


def att2(long_, bias, xt, grid, lds):
    return (f"attention2_kernel<{F16},{long_},{bias},{xt}>", (grid, 1), 512, lds)


def att3(bias, xt, grid, lds):
    return (f"attention3_kernel<{F16},{bias},{xt}>", (grid, 1), 512, lds)


def tail(rw, grid, lds):
    return (f"attention_tail_kernel<{F16},{rw}>", (grid, 1), 256, lds)


BIG = 126976
# (case, kind, arguments, environment, expected dispatches: (kernel, (grid x, y) in workgroups, workgroup size, LDS bytes or None))
CASES = [
    ("qkv", "gemm", dict(M=BIG, N=2304, K=768), {}, [stream(1, 0, 0, 256)]),
    ("qkv ln_rows", "gemm", dict(M=BIG, N=2304, K=768, ln_rows=True), {}, [stream(1, 1, 0, 256)]),
    ("fc1 gelu", "gemm", dict(M=BIG, N=3072, K=768, gelu=True), {}, [stream(1, 0, 1, 256)]),
    ("out_proj resid stats rows", "gemm", dict(M=BIG, N=768, K=768, resid_half=True, stats_out=True, rows_eps=1e-5), {},
     [stream(2, 2, 0, 256), ("ln_rowstats_kernel", None, 256, None)]),
    ("out_proj lnr stats", "gemm", dict(M=BIG, N=768, K=768, lnr=True, stats_out=True), {}, [("lnr_fold_kernel", None, None, None), stream(2, 3, 0, 256)]),
    ("fc2 lnr", "gemm", dict(M=BIG, N=768, K=3072, lnr=True), {}, [("lnr_fold_kernel", None, None, None), stream(2, 1, 0, 256)]),
    ("tap mean", "gemm", dict(M=BIG, N=768, K=3072, resid_half=True, pool_rows=496, pool_mode="mean"), {}, [stream(0, 1, 0, 256)]),
    ("tap max", "gemm", dict(M=BIG, N=768, K=3072, resid_half=True, pool_rows=496, pool_mode="max"), {}, [stream(0, 2, 0, 256)]),
    ("tap cls", "gemm", dict(M=BIG, N=768, K=3072, resid_half=True, pool_rows=496, pool_mode="cls_token"), {}, [stream(0, 3, 0, 256)]),
    ("one clip fc2 split-K", "gemm", dict(M=496, N=768, K=3072, resid_half=True, splitk=True), {},
     [tile128(24, 8), (f"splitk_epilogue_kernel<{F16}>", (372, 1), 256, None)]),
    ("eight clips qkv", "gemm", dict(M=3968, N=2304, K=768), {}, [stream(1, 0, 0, 144)]),
    ("eight clips fc2", "gemm", dict(M=3968, N=768, K=3072), {}, [tile128(186)]),
    ("pinned", "gemm", dict(M=496, N=768, K=768, variant=5), {}, [stream(1, 0, 0, 8)]),
    ("variant 8", "gemm", dict(M=496, N=768, K=768, variant=8), {}, [stream(1, 0, 0, 8)]),
    ("skinny auto", "gemm", dict(M=8208384, N=128, K=64), {}, [(f"gemm_skinny_kernel<{F16},8,2,false,false>", (1024, 1), 256, 16384)]),
    ("skinny 96 x 32", "gemm", dict(M=1000, N=96, K=32, variant=7), {}, [(f"gemm_skinny_kernel<{F16},6,1,false,false>", (8, 1), 256, 6144)]),
    ("refused N", "gemm", dict(M=1000, N=100, K=64), {}, []),
    ("refused K", "gemm", dict(M=1000, N=128, K=40), {}, []),
    ("refused pool_T", "gemm", dict(M=1024, N=768, K=768, pool_rows=32), {}, []),
    ("refused ln_rows variant 3", "gemm", dict(M=1024, N=768, K=768, ln_rows=True, variant=3), {}, []),
    ("skinny off", "gemm", dict(M=8208384, N=128, K=64), {"AVEX_AMD_GEMM_SKINNY": "0"}, [tile128(64128)]),
    ("generic", "gemm", dict(M=BIG, N=2304, K=768), {"AVEX_AMD_GEMM_GENERIC": "1"}, [stream(0, 0, 0, 256)]),
    ("grid 16", "gemm", dict(M=BIG, N=768, K=768), {"AVEX_AMD_GEMM_GRID": "20"}, [stream(1, 0, 0, 16)]),
    ("att 496 bias", "att", dict(T=496, bias=True), {}, [att3("true", "false", 24, 153376)]),
    ("att 496", "att", dict(T=496), {}, [att3("false", "false", 24, 153376)]),
    ("att 513", "att", dict(T=513), {}, [att3("false", "true", 24, 152352), tail(1, 24, 3336)]),
    ("att 513 bias", "att", dict(T=513, bias=True), {}, [att2("true", "true", "false", 24, 158496), tail(1, 24, 3336)]),
    ("att 515", "att", dict(T=515), {}, [att2("true", "false", "true", 48, 150304)]),
    ("att 600", "att", dict(T=600), {}, [att2("true", "false", "false", 48, 158496)]),
    ("att 1025 bias", "att", dict(T=1025, bias=True), {}, [att2("true", "true", "false", 48, 158496), tail(1, 24, 5384)]),
    ("att variant 2", "att", dict(T=496, bias=True), {"AVEX_AMD_ATT_VARIANT": "2"}, [att2("false", "true", "false", 24, 152352)]),
    ("att variant 1", "att", dict(T=496, bias=True), {"AVEX_AMD_ATT_VARIANT": "1"}, [(f"attention_kernel<{F16}>", (24, 1), 1024, 150816)]),
    ("att tail rows 32", "att", dict(T=530, bias=True), {"AVEX_AMD_ATT_TAIL_ROWS": "32"}, [att2("true", "true", "false", 24, 158496), tail(8, 72, 27232)]),
    ("att no tail", "att", dict(T=513), {"AVEX_AMD_ATT_NO_TAIL": "1"}, [att2("true", "false", "true", 48, 150304)]),
    ("att no xt", "att", dict(T=513), {"AVEX_AMD_ATT_NO_XT": "1"}, [att2("true", "false", "false", 24, 158496), tail(1, 24, 3336)]),
    ("att grid 3", "att", dict(T=496, bias=True), {"AVEX_AMD_ATT_GRID": "3"}, [att3("true", "false", 3, 153376)]),
    # one clip through a 1-layer BEATs encoder: out_proj and fc2 with LayerNorm in the split-K epilogue (K = 768: four splits; K = 3072: eight).
    # The last case: its dispatches are looked for in this order among the forward's (the front end has GEMMs of its own)
    ("one clip forward", "beats1", {}, {},
     [tile128(72), att3("true", "false", 12, 153376), tile128(24, 4), (f"splitk_ln_epilogue_kernel<{F16}>", (124, 1), 256, None), tile128(96),
      tile128(24, 8), (f"splitk_ln_epilogue_kernel<{F16}>", (124, 1), 256, None)]),
]
OURS = re.compile(r"gemm256p_kernel|gemm_nt_kernel|gemm_skinny_kernel|splitk_\w*epilogue_kernel|attention\d?_kernel|attention_tail_kernel|ln_rowstats_kernel|lnr_fold_kernel")


def issue() -> None:
    import torch
    sys.path.insert(0, ROOT)
    from avex_amd import synth, kernels as K
    from avex_amd._capi import AvexHipError

    def half(*shape):
        return (torch.rand(*shape, device="cuda") - 0.5).half()

    for name, kind, kw, env, expect in CASES:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            if kind == "gemm":
                kw = dict(kw)
                M, N, Kd = kw.pop("M"), kw.pop("N"), kw.pop("K")
                args = dict(bias=torch.zeros(N, device="cuda"), out_f32=False, out_half=True)
                if kw.pop("resid_half", False):
                    args["resid_half"] = half(M, N)
                if kw.pop("ln_rows", False):
                    args.update(ln_rows=torch.ones(M, 2, device="cuda"), ln_s=torch.zeros(N, device="cuda"))
                if kw.pop("lnr", False):
                    args.update(lnr_y=half(M, N), lnr_rows=torch.ones(M, 2, device="cuda"), lnr_gamma=torch.ones(N, device="cuda"), lnr_beta=torch.zeros(N, device="cuda"))
                args.update(kw)
                try:
                    K.gemm(half(M, Kd), half(N, Kd), **args)
                    print(f"{name}: launched")
                except AvexHipError as e:
                    print(f"{name}: refused: {e}")
            elif kind == "att":
                T, B, H = kw["T"], 2, 12
                tab = torch.zeros(H, 2 * T - 1, device="cuda") if kw.get("bias") else None
                K.attention(half(B * T, 3 * H * 64), B, T, H, tab, None, None, None)
                print(f"{name}: launched")
            else:
                cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=1)
                enc = K.BeatsEncoder(cfg, synth.beats_state_dict(cfg, seed=5), operand_dtype="f16", residual="half")
                enc.forward(torch.from_numpy(synth.noise_clips(1, 160000, seed=9)).cuda(), want_features=True)
                print(f"{name}: launched")
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def plain_name(n: str) -> str:
    """kernel<template arguments> of a trace's kernel name, mangled (c++filt does not know _Float16) or demangled."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", n)
    if not m:
        return re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", "")).replace(" ", "").replace(".kd", "")
    k = m.end() + int(m.group(1))
    name, rest, args = n[m.end():k], n[k:], []
    if rest.startswith("I"):
        for t in re.finditer(r"DF16_|DF16b|L[ib]\d+E|E", rest[1:]):
            if t.group() == "E":
                break
            args.append({"DF16_": "_Float16", "DF16b": "__bf16"}.get(t.group()) or (t.group()[2:-1] if t.group()[1] == "i" else ("false", "true")[int(t.group()[2:-1])]))
    return name + ("<" + ",".join(args) + ">" if args else "")


def dispatches(path):
    """[(kernel<args>, (grid x, y) in workgroups, workgroup size, LDS bytes)] of the trace's GEMM / attention dispatches, in start order."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = {n: plain_name(n) for n in {r["Kernel_Name"] for r in rows}}
    res = []
    for r in rows:
        n = names[r["Kernel_Name"]]
        if not OURS.search(n):
            continue
        wx, wy = int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"])
        res.append((n, (int(r["Grid_Size_X"]) // wx, int(r["Grid_Size_Y"]) // wy), wx * wy, int(r["LDS_Block_Size"])))
    return res


def check(path, against) -> int:
    got = dispatches(path)
    bad, i = 0, 0
    for name, kind, _, _, expect in CASES:
        for want in expect:
            def fits(g):      # (a trace that reports LDS 0 for a kernel with dynamic LDS reports the static part only: nothing to hold the bytes against)
                return g[0] == want[0] and all(w is None or w == x for w, x in zip(want[1:3], g[1:3])) and (want[3] is None or g[3] == 0 or want[3] <= g[3] < want[3] + 512)
            while kind == "beats1" and i < len(got) and not fits(got[i]):
                i += 1
            if i >= len(got):
                print(f"MISSING {name}: {want}")
                bad += 1
                continue
            g = got[i]
            i += 1
            ok = fits(g)
            print(f"{'ok  ' if ok else 'FAIL'} {name:28s} {g[0]:48s} grid {g[1][0]}x{g[1][1]} wg {g[2]} lds {g[3]}" + ("" if ok else f"   expected {want}"))
            bad += not ok
        if not expect:
            print(f"ok   {name:28s} (no dispatch)")
    if i != len(got) and CASES[-1][1] != "beats1":
        print(f"FAIL {len(got) - i} dispatches beyond the table: {got[i:][:5]}")
        bad += 1
    if against:
        other = dispatches(against)
        same = other == got
        print(f"{len(got)} dispatches here, {len(other)} in {against}: " + ("identical (kernel, grid, workgroup, LDS)" if same else "DIFFERENT"))
        if not same:
            for k, (a, b) in enumerate(zip(got, other)):
                if a != b:
                    print(f"  dispatch {k}: {a} / {b}")
            bad += 1
    print("dispatch_trace: " + ("all as expected" if not bad else f"{bad} mismatches"))
    return 1 if bad else 0


if __name__ == "__main__":
    if "--check" in sys.argv:
        path = sys.argv[sys.argv.index("--check") + 1]
        against = sys.argv[sys.argv.index("--against") + 1] if "--against" in sys.argv else None
        sys.exit(check(path, against))
    issue()
