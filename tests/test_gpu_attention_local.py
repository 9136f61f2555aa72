"""Attention per query row and head (attention16.hip, attention.hip, attention_hd.hip, mha_f32 of probe.hip).

The attention tests of test_gpu_kernels.py / test_gpu_probes.py compare with fp64 through ONE rel-L2 over the whole output: about 10^4
(clip, token, head) segments are averaged, and an error confined to a few of them disappears (test_attention_cpu.py shows it).  Here:

  a. per-segment parity: every segment's own relative error against fp64.  The bar is 2 x the worst segment of ``_attention_ref.emulate``
     (fp64 with the kernel's documented operand-type roundings) on the SAME inputs, computed in the test.  Factor 2: device and emulation
     draw different patterns of the same roundings (another softmax reference gives other mantissas), and the maximum of such a statistic
     over 10^3 .. 10^4 segments moves by tens of percent between draws, not by a factor; what the emulation leaves out is fp32-level
     (accumulation order, one ulp of the hardware exp2: about 2^-24 sqrt(T)).
  b. selector: inputs for which query i attends to exactly one key pi(i) != i (``selector_case``); every output element must equal
     V[pi(i)] within the two roundings a kernel may apply to it (P, and the store): 2^-11 + 2^-11 = 2^-10 of |v| for f16, 2^-8 + 2^-8
     = 2^-7 for bf16.  (Not bit equality: the division is by the unrounded row sum.)
  c. range paths: scores that start 60 below zero, sit at -40 throughout, differ between the rows of one 16-query block, or follow a
     fully padded first key tile -- the branches of the streamed kernels' deferred softmax reference that gaussian scores and the
     upward ramp of test_attention_large_logits never enter.  Measured as in (a).

Every test prints ``RATIO <group> <case> ...``: (device worst segment) / (emulation worst segment), the table of DESIGN.md section 6.
"""
import functools

import numpy as np
import pytest
import torch

import _attention_ref as A

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SELECTOR_REL = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
# mha_f32 on selector inputs: the target's exponential is exp(0) = 1 exactly and every other key weighs under 2^-27 (selector_case), so what
# is left is the fp32 arithmetic behind it -- the row sum, its reciprocal, the product with it: half an ulp (2^-24) each -- and the
# off-target rows (under 2^-24 |v|, test_attention_cpu.py): 4 ulp = 2^-21 covers the four with a factor 2.
SELECTOR_REL_F32 = 2.0 ** -21
MHA_FACTOR = 4.0      # fp32 kernels: the margin test_gpu_search.py gives its fp32 products for summation order


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype)


def _tdt(name):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]


def _pad_dev(pad):
    return None if pad is None else _dev(pad.astype(np.uint8), torch.uint8)


def _host(out):
    return out.float().cpu().numpy().astype(np.float64)


def _check_segments(out, ref, emu, B, T, H, D, group, case, factor=2.0):
    """The device's worst segment against ``factor`` x the emulation's, both against fp64."""
    err_e, n_floor = A.segment_errors(emu, ref, H, D)
    A.assert_floor_cap(n_floor, err_e.size)
    err_d, _ = A.segment_errors(out, ref, H, D)
    worst_e, _ = A.worst_segment(err_e)
    worst_d, (r, h) = A.worst_segment(err_d)
    ratio = f"{worst_d / worst_e:.2f}" if worst_e > 0.0 else ("1.00 (both exact)" if worst_d == 0.0 else "inf")
    print(f"RATIO {group} {case} device {worst_d:.3e} emulation {worst_e:.3e} ratio {ratio}")
    n_bad = int((~(err_d <= factor * worst_e)).sum())
    assert worst_d <= factor * worst_e, (f"{group} {case}: {n_bad} of {err_d.size} segments above the bar; worst: clip {r // T} token {r % T} head {h}: "
                                         f"{worst_d:.3e} against {factor:g} x {worst_e:.3e} (the emulation's own worst segment)")


# ---- shared inputs and references (computed once per shape, never changed) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _enc_params(H, kind="random"):
    gw, gb = A.gate_params()
    if kind == "selector":
        table, ga = A.head_params(H, table_clip=A.SELECTOR_TABLE_CLIP)
    elif kind == "range":
        table, ga = A.head_params(H, table_std=A.RANGE_TABLE_STD, table_clip=A.RANGE_TABLE_CLIP)
    else:
        table, ga = A.head_params(H)
    return table, gw, gb, ga


@functools.lru_cache(maxsize=8)
def _toeplitz(kind, H, T):
    return A.toeplitz(_enc_params(H, kind)[0], T, 320, 800)


@functools.lru_cache(maxsize=4)
def _enc_case(B, T, dtype, with_table, masked):
    """(qkv, pad, fp64 reference) of a gaussian encoder case."""
    H = A.ENC_H
    qkv = A.random_case(B, T, H, 64, dtype)
    pad = A.pad_mask(B, T) if masked else None
    table, gw, gb, ga = _enc_params(H) if with_table else (None, None, None, None)
    return qkv, pad, A.attention_ref(qkv, B, T, H, table, gw, gb, ga, key_pad=pad)


def _enc_emulation(B, T, dtype, with_table, masked, **roundings):
    qkv, pad, _ = _enc_case(B, T, dtype, with_table, masked)
    table, gw, gb, ga = _enc_params(A.ENC_H) if with_table else (None, None, None, None)
    return A.emulate(qkv, B, T, A.ENC_H, 64, dtype, table=table, gw=gw, gb=gb, ga=ga, key_pad=pad, **roundings)


def _run_attention(qkv, B, T, H, dtype, kind, with_table, with_gate, pad):
    from avex_amd import kernels as K
    table, gw, gb, ga = _enc_params(H, kind)
    tab = _dev(_toeplitz(kind, H, T)) if with_table else None
    gate = (_dev(gw), _dev(gb), _dev(ga)) if with_table and with_gate else (None, None, None)
    return _host(K.attention(_dev(qkv, _tdt(dtype)), B, T, H, tab, *gate, key_pad=_pad_dev(pad)))


def _masks(B, T):
    return (False, True) if A.pad_mask(B, T) is not None else (False,)


# ---- a. per-segment parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["1", "2", "3"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", A.ENC_T_TABLE)
def test_segment_parity_gated_bias(built_lib, T, dtype, variant, monkeypatch):
    """Gate, bias table, and (second launch) a key mask with a padded first key tile, a padded tail over whole key tiles and a clip with one
    unpadded key; several (head, clip) items per workgroup, each run crossing a head seam."""
    monkeypatch.setenv("AVEX_AMD_ATT_VARIANT", variant)
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(A.ENC_GRID))
    B, H = A.ENC_B, A.ENC_H
    for masked in _masks(B, T):
        qkv, pad, ref = _enc_case(B, T, dtype, True, masked)
        out = _run_attention(qkv, B, T, H, dtype, "random", True, True, pad)
        emu = _enc_emulation(B, T, dtype, True, masked, **A.KERNEL_ROUNDINGS[variant])
        _check_segments(out, ref, emu, B, T, H, 64, "gated_bias", f"v{variant} {dtype} T={T} mask={int(masked)}")


_PLAIN = [(499, 0, v) for v in ("1", "2", "3")] + [(T, rows, v) for T, rows in A.ENC_T_PLAIN[1:] for v in ("2", "3")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,tail,variant", _PLAIN)
def test_segment_parity_without_a_table(built_lib, T, tail, variant, dtype, monkeypatch):
    """No bias table (AVES at 499 frames, EAT at 513 tokens): 513 and 544 (with 32 tail rows asked for) take variant 3's nine-tile last
    phase for the first 512 query rows and the tail kernel for the rest; 544 as shipped runs two query blocks of variant 2."""
    monkeypatch.setenv("AVEX_AMD_ATT_VARIANT", variant)
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(A.ENC_GRID))
    if tail:
        monkeypatch.setenv("AVEX_AMD_ATT_TAIL_ROWS", str(tail))
    B, H = A.ENC_B, A.ENC_H
    # beyond 512 tokens the streamed rows run on variant 3's nine-tile form when the tail kernel takes the rest, else on variant 2
    tail_rows = A.tail_rows(T, tail)
    roundings = A.KERNEL_ROUNDINGS[variant if T <= 512 else ("3" if variant == "3" and tail_rows.any() else "2")]
    for masked in _masks(B, T):
        qkv, pad, ref = _enc_case(B, T, dtype, False, masked)
        out = _run_attention(qkv, B, T, H, dtype, "random", False, False, pad)
        emu = _enc_emulation(B, T, dtype, False, masked, tail_rows=tail_rows, **roundings)
        _check_segments(out, ref, emu, B, T, H, 64, "no_table", f"v{variant} {dtype} T={T} tail={tail} mask={int(masked)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,grid", A.ENC_LONG)
def test_segment_parity_long_clips(built_lib, T, grid, dtype, monkeypatch):
    """More than 512 tokens: query blocks of 512, bias windows per phase; the grid makes workgroups start in the middle of an item."""
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(grid))
    B, H = A.ENC_LONG_B, A.ENC_H
    for masked in _masks(B, T):
        qkv, pad, ref = _enc_case(B, T, dtype, True, masked)
        out = _run_attention(qkv, B, T, H, dtype, "random", True, True, pad)
        emu = _enc_emulation(B, T, dtype, True, masked, **A.KERNEL_ROUNDINGS["2"])
        _check_segments(out, ref, emu, B, T, H, 64, "long_clips", f"{dtype} T={T} grid={grid} mask={int(masked)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", A.HD_D)
@pytest.mark.parametrize("T", A.HD_T)
def test_segment_parity_other_head_widths(built_lib, T, D, dtype):
    from avex_amd import kernels as K
    B, H = A.HD_B, A.HD_H
    qkv = A.random_case(B, T, H, D, dtype)
    for pad in (None, A.pad_mask(B, T)):
        out = _host(K.attention_hd(_dev(qkv, _tdt(dtype)), B, T, H, D, key_pad=_pad_dev(pad)))
        ref = A.plain_attention_ref(qkv, B, T, H, D, key_pad=pad)
        emu = A.emulate(qkv, B, T, H, D, dtype, key_pad=pad, **A.KERNEL_ROUNDINGS["hd"])
        _check_segments(out, ref, emu, B, T, H, D, "attention_hd", f"{dtype} D={D} T={T} mask={int(pad is not None)}")


@pytest.mark.parametrize("D", A.MHA_D)
@pytest.mark.parametrize("T", A.HD_T)
def test_segment_parity_mha_f32(built_lib, T, D):
    """probe.hip's fp32 attention core (the matrix-core kernel at head widths 32 / 64 / 96 / 128, the plain one at 48): the same measure,
    the bar 4 x the worst segment of a NumPy fp32 restatement against fp64."""
    from avex_amd import kernels as K
    B, H = A.HD_B, A.HD_H
    qkv = A.random_case(B, T, H, D, "f32")
    for pad in (None, A.pad_mask(B, T)):
        out = _host(K.mha_f32(_dev(qkv).reshape(B, T, 3 * H * D), H, _pad_dev(pad)).reshape(B * T, H * D))
        ref = A.plain_attention_ref(qkv, B, T, H, D, key_pad=pad)
        emu = A.mha_f32_restatement(qkv, B, T, H, D, key_pad=pad)
        _check_segments(out, ref, emu, B, T, H, D, "mha_f32", f"D={D} T={T} mask={int(pad is not None)}", factor=MHA_FACTOR)


# ---- b. selector ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _selector(B, T, H, D, dtype, full):
    """Selector inputs: plain (no bias, gate or mask), or ``full``: mask, and -- head width 64 with a table -- gated bias."""
    if not full:
        return A.selector_case(B, T, H, D, dtype) + (None,)
    pad = A.pad_mask(B, T)
    bias = None
    if full == "bias":
        table, gw, gb, ga = _enc_params(H, "selector")
        bias = dict(table=table, gw=gw, gb=gb, ga=ga)
    return A.selector_case(B, T, H, D, dtype, pad=pad, bias=bias) + (pad,)


def _check_selector(out, qkv, pi, B, T, H, D, rel, what):
    msg = A.selector_mismatch(out, qkv, pi, B, T, H, D, rel)
    assert msg is None, f"{what}: {msg}"


@pytest.mark.parametrize("variant", ["1", "2", "3"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", A.SEL_T_TABLE)
def test_selector_gated_bias(built_lib, T, dtype, variant, monkeypatch):
    """Query i reads key pi(i) and value row pi(i): without bias, gate and mask, and with all three (padded keys repeat targets' codes)."""
    monkeypatch.setenv("AVEX_AMD_ATT_VARIANT", variant)
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(A.ENC_GRID))
    B, H = A.ENC_B, A.ENC_H
    for full in (False, "bias"):
        qkv, pi, _, pad = _selector(B, T, H, 64, dtype, full)
        out = _run_attention(qkv, B, T, H, dtype, "selector", bool(full), bool(full), pad)
        _check_selector(out, qkv, pi, B, T, H, 64, SELECTOR_REL[dtype], f"v{variant} {dtype} T={T} bias/gate/mask={bool(full)}")


@pytest.mark.parametrize("variant", ["2", "3"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,tail", A.SEL_T_PLAIN)
def test_selector_without_a_table(built_lib, T, tail, dtype, variant, monkeypatch):
    """513 and 544 tokens: targets in the ninth key tile, queries in the tail kernel."""
    monkeypatch.setenv("AVEX_AMD_ATT_VARIANT", variant)
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(A.ENC_GRID))
    if tail:
        monkeypatch.setenv("AVEX_AMD_ATT_TAIL_ROWS", str(tail))
    B, H = A.ENC_B, A.ENC_H
    for full in (False, "mask"):
        qkv, pi, _, pad = _selector(B, T, H, 64, dtype, full)
        out = _run_attention(qkv, B, T, H, dtype, "selector", False, False, pad)
        _check_selector(out, qkv, pi, B, T, H, 64, SELECTOR_REL[dtype], f"v{variant} {dtype} T={T} mask={bool(full)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,grid", A.SEL_T_LONG)
def test_selector_long_clips(built_lib, T, grid, dtype, monkeypatch):
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(grid))
    B, H = A.ENC_LONG_B, A.ENC_H
    for full in (False, "bias"):
        qkv, pi, _, pad = _selector(B, T, H, 64, dtype, full)
        out = _run_attention(qkv, B, T, H, dtype, "selector", bool(full), bool(full), pad)
        _check_selector(out, qkv, pi, B, T, H, 64, SELECTOR_REL[dtype], f"{dtype} T={T} grid={grid} bias/gate/mask={bool(full)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", A.HD_D)
@pytest.mark.parametrize("T", A.SEL_HD_T)
def test_selector_other_head_widths(built_lib, T, D, dtype):
    from avex_amd import kernels as K
    B, H = A.HD_B, A.HD_H
    for full in (False, "mask"):
        qkv, pi, _, pad = _selector(B, T, H, D, dtype, full)
        out = _host(K.attention_hd(_dev(qkv, _tdt(dtype)), B, T, H, D, key_pad=_pad_dev(pad)))
        _check_selector(out, qkv, pi, B, T, H, D, SELECTOR_REL[dtype], f"attention_hd {dtype} D={D} T={T} mask={bool(full)}")


@pytest.mark.parametrize("D", A.MHA_D)
@pytest.mark.parametrize("T", A.SEL_HD_T)
def test_selector_mha_f32(built_lib, T, D):
    from avex_amd import kernels as K
    B, H = A.HD_B, A.HD_H
    for full in (False, "mask"):
        qkv, pi, _, pad = _selector(B, T, H, D, "f32", full)
        out = _host(K.mha_f32(_dev(qkv).reshape(B, T, 3 * H * D), H, _pad_dev(pad)).reshape(B * T, H * D))
        _check_selector(out, qkv, pi, B, T, H, D, SELECTOR_REL_F32, f"mha_f32 D={D} T={T} mask={bool(full)}")


# ---- c. range paths ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _range(pattern, D, dtype):
    B, H, T = A.RANGE_B, A.RANGE_H, A.RANGE_T
    qkv, pad = A.range_case(pattern, B, T, H, D, dtype)
    table = _enc_params(H, "range")[0] if D == 64 else None
    A.assert_range_case(pattern, qkv, B, T, H, D, table=table)
    ref = A.attention_ref(qkv, B, T, H, table, None, None, None, key_pad=pad) if D == 64 else A.plain_attention_ref(qkv, B, T, H, D, key_pad=pad)
    return qkv, pad, table, ref


@pytest.mark.parametrize("variant", ["1", "2", "3"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern", A.RANGE_PATTERNS)
def test_range_paths(built_lib, pattern, dtype, variant, monkeypatch):
    """A negative first reference that moves; one that never moves; rows of one 16-query block that disagree about moving theirs; a row left
    without a reference by a padded first key tile and given a negative one by the second (``_attention_ref.range_case``)."""
    monkeypatch.setenv("AVEX_AMD_ATT_VARIANT", variant)
    monkeypatch.setenv("AVEX_AMD_ATT_GRID", str(A.RANGE_GRID))
    B, H, T = A.RANGE_B, A.RANGE_H, A.RANGE_T
    qkv, pad, table, ref = _range(pattern, 64, dtype)
    out = _run_attention(qkv, B, T, H, dtype, "range", True, False, pad)
    assert np.isfinite(out).all()
    emu = A.emulate(qkv, B, T, H, 64, dtype, table=table, key_pad=pad, **A.KERNEL_ROUNDINGS[variant])
    _check_segments(out, ref, emu, B, T, H, 64, "range_paths", f"v{variant} {dtype} {pattern}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern", A.RANGE_PATTERNS[:2])
def test_range_paths_other_head_widths(built_lib, pattern, dtype):
    from avex_amd import kernels as K
    B, H, T, D = A.RANGE_B, A.RANGE_H, A.RANGE_T, 96
    qkv, pad, _, ref = _range(pattern, D, dtype)
    out = _host(K.attention_hd(_dev(qkv, _tdt(dtype)), B, T, H, D, key_pad=_pad_dev(pad)))
    assert np.isfinite(out).all()
    emu = A.emulate(qkv, B, T, H, D, dtype, key_pad=pad, **A.KERNEL_ROUNDINGS["hd"])
    _check_segments(out, ref, emu, B, T, H, D, "range_paths", f"attention_hd {dtype} D={D} {pattern}")
