"""The row kernels of avex_amd/csrc/elementwise.hip off the model shapes, one kernel at a time through the C ABI (ABI 19): both LayerNorm
kernels and the fused LayerNorm + pool, the pooling kernels, the GLU gate, the casts, row zeroing, the row sums, the LayerNorm fold
vectors, the Toeplitz bias table and the EAT token assembly.

Inputs come from avex_amd.synth; half inputs are rounded on the CPU first, so a kernel sees exactly the numbers its reference sees.
References are tests/_rows_ref.py (fp64, or fp32 in the kernel's own order where the statement is about bits; pinned against torch by
tests/test_rows_ref_cpu.py).  Every case with a leading dimension wider than its rows fills its buffers with a sentinel and asserts, bit for
bit, that the gaps between the rows and the guard rows behind the last one are untouched.

Measured bars (the worst error over all cases of the test on an MI355X, asserted at four times that; DESIGN.md has the table):
    glu_swish       delta = 1.720e-7 (f16) / 9.528e-8 (bf16), the fp32 slack of rcp and exp2 in  |got - ref| <= ulp_T(ref) / 2 + delta |ref|
    layernorm_pool  5.534e-7, max |got - fp64| over the [B, C] outputs
    layernorm       bf16 input needs no bar of its own: the worst of all 33 cases is 1.032e-6 (bf16: 9.9e-7) under the 5e-6 of test_layernorm."""
import math

import numpy as np
import pytest
import torch

import _rows_ref as R
from _attention_ref import toeplitz as _toeplitz_direct
from _util import max_abs, rel_l2, round_half
from avex_amd import synth
from oracle import beats_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SENT = -1984.0          # exact in f16, bf16 and fp32: a buffer filled with it shows every element a kernel wrote
ERR_INVALID = -1

# measured on an MI355X (first run of this file), each the worst over every case of its test; the asserts use four times these
GLU_DELTA_MEASURED = {"f16": 1.720e-7, "bf16": 9.528e-8}      # (33, 3072) in both types; most shapes show no slack at all
LNPOOL_MEASURED = 5.534e-7                                   # C = 760, bf16
LN_WORST_MEASURED = 1.032e-6                                 # half kernel, C = 520, f16
LN_TOL = 5e-6           # fp32 LayerNorm output against fp64 for the N(0.5, 2) rows of test_gpu_kernels.py::test_layernorm (its bar)


def _K():
    from avex_amd import kernels
    return kernels


def _tdt(name):
    return torch.float16 if name == "f16" else torch.bfloat16


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype)


def _np(t):
    return t.float().cpu().numpy() if t.dtype != torch.float32 else t.cpu().numpy()


def _bits(t):
    """A tensor's bit patterns as a NumPy integer array."""
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_f32(got, want):
    return got.shape == want.shape and np.array_equal(_f32_bits(got), _f32_bits(want))


def _full(shape, dtype, value=SENT):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _untouched(buf, M, Cc, what):
    """The gaps beside the first Cc columns of rows < M, and every row from M on, still hold the sentinel's bits."""
    want = _bits(_full((1,), buf.dtype))[0]
    b = _bits(buf)
    b = b.reshape(1, -1) if b.ndim == 1 else b
    assert (b[:M, Cc:] == want).all(), (what, "gap columns written")
    assert (b[M:] == want).all(), (what, "guard rows written")


def _strided(x, ld, dtype, fill=float("nan")):
    """x [M, C] in a [M, ld] device buffer of `dtype`, NaN beside its own columns (a kernel that reads a gap shows it)."""
    M, Cc = x.shape
    buf = torch.full((M, ld), fill, dtype=dtype, device="cuda")
    buf[:, :Cc] = _dev(x, dtype)
    return buf


# ---- layernorm ---------------------------------------------------------------------------------------------------------------------------
LN_M = [1, 7, 8, 9, 333]
LN_ROWS = 333
CONST_ROW, ZERO_ROW, BIG_ROW = 2, 3, 4      # rows of every input with M > 4 (M = 1 has row 0 only, an ordinary row)

LN_CASES = ([("f32", C_, "f16") for C_ in (4, 252, 256, 260, 768, 1020)] + [("f32", 1024, "f16"), ("f32", 256, "bf16"), ("f32", 1024, "bf16")]
            + [("half", C_, dt) for C_ in (8, 248, 256, 264, 512, 520, 760, 768) for dt in DTYPES]
            + [("generic", C_, dt) for C_ in (772, 1024) for dt in DTYPES] + [("generic_ld", 768, dt) for dt in DTYPES])


def _ln_inputs(path, Cc, dtype):
    x = synth.normal(f"rows_ln{Cc}", (LN_ROWS, Cc), 2.0) + np.float32(0.5)
    x[CONST_ROW] = 3.25
    x[ZERO_ROW] = 0.0
    if path == "f32":
        x[BIG_ROW] = np.float32(1e4) + synth.normal(f"rows_lnbig{Cc}", (Cc,), 1.0)
    else:
        x = round_half(x, dtype)
    w = (1.0 + synth.normal("rows_lnw", (Cc,), 0.1)).astype(np.float32)
    b = synth.normal("rows_lnb", (Cc,), 0.1).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("path,Cc,dtype", LN_CASES)
def test_layernorm_paths(built_lib, path, Cc, dtype):
    """avexhip_layernorm on each of its three paths -- fp32 input (generic kernel, one wave per row), half input (half kernel, one half-wave
    per row: C % 8 == 0, C <= 768, ld_in % 8 == 0) and half input that the launcher sends to the generic kernel (C = 772, C = 1024, or
    ld_in = C + 4) -- at row counts around the 4 / 8 rows of a workgroup, with leading dimensions equal to C and wider, with both outputs, the
    fp32 one alone and the half one alone.  The row widths put the last chunk of a lane everywhere: C / 4 resp. C / 8 below, at and above a
    multiple of the 64 resp. 32 lanes.

    fp32 output against the fp64 two-pass LayerNorm at 5e-6 (test_layernorm's bar, same input distribution); a constant row and an all-zero
    row give the bias exactly (their centred values are exactly 0); the half output is the rounding of the fp32 output, bit for bit.

    The row with mean 1e4 and unit spread (fp32 input): the kernel's mean is sum / C with at most 12 roundings of 2^-24 on the way to the sum
    (4 chunk sums of depth 2, 4 sequential adds, 6 butterfly levels; first order, every partial sum <= sum |x|) and one in the division:
    |mean - mu| <= 6.5 * 2^-23 * |x|max.  x - mean is then exact (both within a factor 2), so every centred value is off by that one shift,
    and the output by shift * rstd * |w|.  The variance moves by shift^2 (the centred values sum to 0): 4e-5 relative here, far below the
    shift's own effect.  With 1.5 * 2^-23 * |x|max * rstd left for everything else (rstd, the multiply-adds: 5e-6 on a unit-variance row):
        |got - ref| <= 8 * |x|max * 2^-23 * rstd * max|w|."""
    K = _K()
    td = _tdt(dtype)
    x, w, b = _ln_inputs(path, Cc, dtype)
    wd, bd = _dev(w), _dev(b)
    ref = R.layer_norm(x, w, b, 1e-5)
    in_t = torch.float32 if path == "f32" else td
    lds = [(Cc, Cc, Cc), (Cc + 8, Cc + 4, Cc + 8)] if path != "generic_ld" else [(Cc + 4, Cc, Cc), (Cc + 4, Cc + 4, Cc + 8)]
    ordinary = np.ones(LN_ROWS, bool)
    ordinary[[CONST_ROW, ZERO_ROW]] = False
    if path == "f32":
        ordinary[BIG_ROW] = False
    worst = 0.0
    for M in LN_M:
        for ld_in, ldo, ldh in lds:
            xin = _strided(x[:M], ld_in, in_t)
            for want32, wanth in ((True, True), (True, False), (False, True)):
                what = (path, Cc, dtype, M, ld_in, ldo, ldh, want32, wanth)
                o32 = _full((M + 2, ldo), torch.float32) if want32 else None
                oh = _full((M + 2, ldh), td) if wanth else None
                r32, rh = K.layernorm(xin, wd, bd, 1e-5, half_dtype=dtype, want_f32=want32, want_half=wanth, ld_in=ld_in,
                                      out_f32=o32, out_half=oh)
                assert (r32 is o32) and (rh is oh)
                if want32:
                    _untouched(o32, M, Cc, what)
                    got = o32[:M, :Cc].cpu().numpy()
                    keep = ordinary[:M]
                    err = max_abs(got[keep], ref[:M][keep]) if keep.any() else 0.0
                    worst = max(worst, err)
                    assert err < LN_TOL, (what, err)
                    if M > BIG_ROW:
                        assert _same_f32(got[CONST_ROW], b) and _same_f32(got[ZERO_ROW], b), (what, "constant / zero row is not the bias")
                        if path == "f32":
                            rstd = float(R.row_rstd(x[BIG_ROW], 1e-5)[0])
                            bar = 8.0 * float(np.abs(x[BIG_ROW]).max()) * R.F32_ULP * rstd * float(np.abs(w).max())
                            assert max_abs(got[BIG_ROW], ref[BIG_ROW]) <= bar, (what, "mean-1e4 row", max_abs(got[BIG_ROW], ref[BIG_ROW]), bar)
                    if wanth:
                        full32 = got
                if wanth:
                    _untouched(oh, M, Cc, what)
                    goth = _np(oh[:M, :Cc])
                    if want32:
                        assert _same_f32(goth, round_half(full32, dtype)), (what, "half output is not the rounding of the fp32 output")
                        both_h = goth
                    else:      # alone: the same bits as beside the fp32 output (whose rounding it was shown to be)
                        assert _same_f32(goth, both_h), (what, "half output alone differs from the one beside the fp32 output")
    print(f"layernorm {path} C={Cc} {dtype}: worst max|got - fp64| over ordinary rows {worst:.3e}")


def _ln_call(lib, x32, xh, ld_in, w, b, M, Cc, o32, ldo, oh, ldh, code=0):
    p = lambda t: None if t is None else int(t.data_ptr())      # noqa: E731
    return lib.avexhip_layernorm(p(x32), p(xh), ld_in, p(w), p(b), 1e-5, M, Cc, p(o32), ldo, p(oh), ldh, code, None)


def test_layernorm_refusals(built_lib):
    """What the launcher refuses comes back as AVEXHIP_ERR_INVALID with a message, and nothing is written."""
    M = 5
    x32 = _full((M, 1040), torch.float32, 1.0)
    xh = _full((M, 1040), torch.float16, 1.0)
    w, b = _full((1040,), torch.float32, 1.0), _full((1040,), torch.float32, 0.0)
    cases = {
        "C % 4": dict(x32=x32, xh=None, ld_in=1040, Cc=254, ldo=1040, ldh=1040),
        "C = 1028": dict(x32=x32, xh=None, ld_in=1040, Cc=1028, ldo=1040, ldh=1040),
        "ld_in % 4": dict(x32=x32, xh=None, ld_in=1038, Cc=256, ldo=1040, ldh=1040),
        "ldo % 4": dict(x32=x32, xh=None, ld_in=1040, Cc=256, ldo=1038, ldh=1040),
        "ldh % 4": dict(x32=None, xh=xh, ld_in=1040, Cc=256, ldo=1040, ldh=1038),
        "both inputs": dict(x32=x32, xh=xh, ld_in=1040, Cc=256, ldo=1040, ldh=1040),
        "no input": dict(x32=None, xh=None, ld_in=1040, Cc=256, ldo=1040, ldh=1040),
    }
    for name, kw in cases.items():
        o32, oh = _full((M, 1040), torch.float32), _full((M, 1040), torch.float16)
        rc = _ln_call(built_lib, kw["x32"], kw["xh"], kw["ld_in"], w, b, M, kw["Cc"], o32, kw["ldo"], oh, kw["ldh"])
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, (name, rc)
        assert built_lib.avexhip_last_error().decode().startswith("layernorm:"), name
        _untouched(o32, 0, 0, name)
        _untouched(oh, 0, 0, name)
    rc = _ln_call(built_lib, x32, None, 1040, w, b, M, 256, None, 1040, None, 1040)
    assert rc == ERR_INVALID and "no output" in built_lib.avexhip_last_error().decode()


# ---- layernorm_pool ----------------------------------------------------------------------------------------------------------------------
LNP_T = [1, 31, 32, 33, 63, 64, 65, 129, 496]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc", [8, 264, 760, 768])
def test_layernorm_pool(built_lib, dtype, Cc):
    """The fused final LayerNorm + token mean against the fp64 mean of the fp64 LayerNorm.  Token counts around the 32 half-waves of a
    workgroup (the first row of every half-wave), the second row in flight (32 .. 63) and the 64-row stride; widths with one chunk, a partly
    filled second and third chunk, and all three full; leading dimension C and C + 8; a batch of 3 and each clip alone: a clip's bits do not
    depend on the batch, and a second run gives the same bits."""
    K = _K()
    td = _tdt(dtype)
    w = (1.0 + synth.normal("rows_lnw", (Cc,), 0.1)).astype(np.float32)
    b = synth.normal("rows_lnb", (Cc,), 0.1).astype(np.float32)
    wd, bd = _dev(w), _dev(b)
    worst = 0.0
    for T in LNP_T:
        x = round_half(synth.normal(f"rows_lnp{T}_{Cc}", (3, T, Cc), 2.0) + np.float32(0.5), dtype)
        ref = R.layer_norm_pool(x, w, b, 1e-5)
        for ld in (Cc, Cc + 8):
            xin = _strided(x.reshape(3 * T, Cc), ld, td)
            out = K.layernorm_pool(xin, wd, bd, 1e-5, 3, T)
            got = out.cpu().numpy()
            err = max_abs(got, ref)
            worst = max(worst, err)
            assert err <= 4.0 * LNPOOL_MEASURED, (dtype, Cc, T, ld, err)
            assert np.array_equal(_bits(K.layernorm_pool(xin, wd, bd, 1e-5, 3, T)), _bits(out)), (T, ld, "second run differs")
            for clip in range(3):
                alone = K.layernorm_pool(xin[clip * T:(clip + 1) * T].contiguous(), wd, bd, 1e-5, 1, T)
                assert np.array_equal(_bits(alone)[0], _bits(out)[clip]), (dtype, Cc, T, ld, clip, "a clip alone differs from the clip in a batch")
    print(f"layernorm_pool C={Cc} {dtype}: worst max|got - fp64| {worst:.3e}")


def test_layernorm_pool_refusals(built_lib):
    from avex_amd._capi import AvexHipError
    K = _K()
    for Cc in (776, 260, 4):
        x = _full((64, Cc), torch.float16, 1.0)
        with pytest.raises(AvexHipError, match="layernorm_pool"):
            K.layernorm_pool(x, _full((Cc,), torch.float32, 1.0), _full((Cc,), torch.float32, 0.0), 1e-5, 1, 64)
    x = _full((64, 260), torch.float16, 1.0)      # a leading dimension that is no multiple of 8 under a legal width
    with pytest.raises(AvexHipError, match="layernorm_pool"):
        K.layernorm_pool(x, _full((256,), torch.float32, 1.0), _full((256,), torch.float32, 0.0), 1e-5, 1, 64)


# ---- mean_pool / agg_pool / pool_reduce --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 496])
def test_mean_pool_bits(built_lib, T):
    """mean_pool_kernel holds the bits of its stated order (four token phases, each in increasing t, (p0 + p1) + (p2 + p3), / T) at widths
    below, at and above its 64-column blocks and with fewer tokens than phases; avexhip_agg_pool mode 1 is the same kernel."""
    K = _K()
    for Cc in (1, 63, 64, 65, 768):
        x = synth.normal(f"rows_mp{T}_{Cc}", (3, T, Cc), 1.0)
        want = R.mean_pool_f32(x)
        got = K.mean_pool(_dev(x)).cpu().numpy()
        assert _same_f32(got, want), (T, Cc, int((_f32_bits(got) != _f32_bits(want)).sum()))
        assert _same_f32(K.agg_pool(_dev(x), 1).cpu().numpy(), want), (T, Cc, "agg_pool mode 1")
        assert _same_f32(K.mean_pool(_dev(x[1:2])).cpu().numpy(), want[1:2]), (T, Cc, "one clip")


def test_mean_pool_nan_stays_in_its_clip_and_column(built_lib):
    K = _K()
    x = synth.normal("rows_mpnan", (3, 7, 65), 1.0)
    x[1, 5, 64] = np.nan
    got = K.mean_pool(_dev(x)).cpu().numpy()
    where = np.argwhere(np.isnan(got))
    assert where.tolist() == [[1, 64]]
    assert _same_f32(np.nan_to_num(got), np.nan_to_num(R.mean_pool_f32(x)))


@pytest.mark.parametrize("T", [1, 2, 496])
def test_agg_pool_max_and_first(built_lib, T):
    """Mode 2 is the maximum over a clip's rows -- on all-negative data with -inf rows, where a maximum started at 0 or at a finite floor
    shows -- and mode 3 its first row, both exact, at widths around the 256-column blocks."""
    K = _K()
    for Cc in (1, 255, 256, 257, 768):
        x = -np.abs(synth.normal(f"rows_ap{T}_{Cc}", (2, T, Cc), 1.0)) - np.float32(0.5)
        x[0, T // 2] = -np.inf                 # a whole row
        x[1, :, Cc // 2] = -np.inf             # a whole column: its maximum is -inf
        xd = _dev(x)
        want = torch.from_numpy(x).max(dim=1)[0].numpy()
        assert np.array_equal(want, R.max_pool(x))
        assert _same_f32(K.agg_pool(xd, 2).cpu().numpy(), want), (T, Cc, "max")
        assert _same_f32(K.agg_pool(xd, 3).cpu().numpy(), x[:, 0]), (T, Cc, "first row")


def test_max_pool_keeps_nan(built_lib):
    """torch.max over a dimension keeps a NaN; so do avexhip_agg_pool mode 2 and avexhip_pool_reduce_mode mode 1 (fmaxf dropped it: the
    pooled embedding of a poisoned clip came out finite).  The NaN first, in the middle and last in the order of the reduction."""
    K = _K()
    T, Cc = 5, 257
    x = synth.normal("rows_apnan", (2, T, Cc), 1.0)
    x[0, 0, 3] = np.nan
    x[0, 2, 255] = np.nan
    x[1, T - 1, 256] = np.nan
    got = K.agg_pool(_dev(x), 2).cpu().numpy()
    want = torch.from_numpy(x).max(dim=1)[0].numpy()
    assert np.argwhere(np.isnan(got)).tolist() == [[0, 3], [0, 255], [1, 256]]
    assert _same_f32(np.nan_to_num(got), np.nan_to_num(want))
    # pool_reduce: two clips of 96 rows = three 64-row blocks; clip 0 owns slot 0 of blocks 0 and 1, clip 1 slot 1 of block 1 and slot 0
    # of block 2; the two slots nothing owns hold NaN and must not be read
    N = 257
    part = synth.normal("rows_prnan", (3, 2, N), 1.0)
    part[0, 1] = np.nan
    part[2, 1] = np.nan
    part[0, 0, 7] = np.nan            # clip 0: NaN in its first block, a finite value behind it
    part[1, 0, 256] = np.nan          # clip 0: NaN in its last block
    part[1, 1, 100] = np.nan          # clip 1: NaN in its first block
    want = np.stack([R.max_pool(part[[0, 1], 0][None])[0], R.max_pool(np.stack([part[1, 1], part[2, 0]])[None])[0]])
    got = K.pool_reduce(_dev(part), 2, 96, mode=1).cpu().numpy()
    assert np.argwhere(np.isnan(got)).tolist() == [[0, 7], [0, 256], [1, 100]]
    assert _same_f32(np.nan_to_num(got), np.nan_to_num(want))
    # the mean of the same blocks: unowned slots unread here too
    part2 = np.nan_to_num(part, nan=0.0)
    part2[0, 1] = np.nan
    part2[2, 1] = np.nan
    mean = K.pool_reduce(_dev(part2), 2, 96, mode=0).cpu().numpy()
    assert np.isfinite(mean).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_pooled_max_keeps_nan(built_lib, dtype):
    """The pooled-tap epilogue's partial maxima at the smallest shape the planner takes (two clips of 64 rows; pool_part exists in the
    256-tile kernel only, which needs N % 256 == 0 and K >= 128, so N = 256 and K = 128): a NaN operand in one row of
    clip 1 makes that clip's pooled maximum NaN in every column and leaves clip 0 alone; an infinite operand against one zero weight makes
    exactly one (clip, column) NaN (inf * 0) beside +inf columns."""
    K = _K()
    td = _tdt(dtype)
    T, N, Kd = 64, 256, 128
    a = round_half(synth.normal("rows_pmA", (2 * T, Kd), 1.0), dtype)
    w = np.abs(round_half(synth.normal("rows_pmW", (N, Kd), 0.1), dtype)) + np.float32(0.0625)
    w = round_half(w, dtype)
    bias = synth.normal("rows_pmb", (N,), 0.3)
    clean = K.gemm(_dev(a, td), _dev(w, td), bias=_dev(bias), out_raw=True, pool_rows=T, pool_mode="max")
    assert torch.equal(clean["pooled"], clean["raw"].reshape(2, T, N).max(dim=1)[0])
    a1 = a.copy()
    a1[T + 37, 5] = np.nan
    got = K.gemm(_dev(a1, td), _dev(w, td), bias=_dev(bias), pool_rows=T, pool_mode="max")["pooled"].cpu().numpy()
    assert np.isnan(got[1]).all() and _same_f32(got[0], clean["pooled"][0].cpu().numpy())
    a2, w2 = a.copy(), w.copy()
    a2[9, 11] = np.inf
    w2[77, 11] = 0.0
    got = K.gemm(_dev(a2, td), _dev(w2, td), bias=_dev(bias), pool_rows=T, pool_mode="max")["pooled"].cpu().numpy()
    assert np.argwhere(np.isnan(got)).tolist() == [[0, 77]]
    assert np.isposinf(np.delete(got[0], 77)).all()
    assert _same_f32(np.delete(got[1], 77), np.delete(clean["pooled"][1].cpu().numpy(), 77))      # (column 77 has another weight row now)


# ---- glu_swish ---------------------------------------------------------------------------------------------------------------------------
GLU_SHAPES = [(1, 8), (255, 8), (256, 8), (257, 8), (3, 264), (33, 3072)]
GLU_GATES = [0.0, 2.0 ** -14, -2.0 ** -14, -20.0, 100.0, -100.0, -65504.0]


def _glu_input(M, F, dtype):
    y = synth.normal(f"rows_glu{M}_{F}", (M, 2 * F), 2.0)
    y[:, F:] *= np.float32(1.5)
    g = y[:, F:].reshape(-1)
    n = len(GLU_GATES)
    g[:n] = GLU_GATES                      # the first work item(s)
    g[-n:] = GLU_GATES[::-1]               # and the last: the item behind a block edge at 257 rows
    y[:, F:] = g.reshape(M, F)
    return round_half(y, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,F", GLU_SHAPES)
def test_glu_swish(built_lib, dtype, M, F):
    """out = a * g * sigmoid(g) against fp64, per element:  |got - ref| <= ulp_T(ref) / 2 + delta * |ref|  -- the rounding to the operand
    type plus the fp32 error of the kernel's rcp and exp2, delta measured (module docstring).  One thread, the block edge at 255 / 256 / 257
    work items, a width with 33 items per row, the model width.  Gates 0, +-2^-14, -20 (result near the f16 subnormals), +-100 and -65504
    (exp2 overflows: rcp gives 0 and the result is a zero with the sign of -a) in the first and in the last work item."""
    K = _K()
    y = _glu_input(M, F, dtype)
    got = _np(K.glu_swish(_dev(y, _tdt(dtype)))).astype(np.float64)
    ref = R.glu_swish(y)
    assert np.isfinite(ref).all() and np.abs(ref).max() < 60000.0
    slack = np.abs(got - ref) - 0.5 * R.half_ulp(ref, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = float(np.max(np.where(ref != 0, np.maximum(slack, 0.0) / np.abs(ref), np.where(slack > 0, np.inf, 0.0))))
    print(f"glu_swish M={M} F={F} {dtype}: delta {delta:.3e}")
    assert delta <= 4.0 * GLU_DELTA_MEASURED[dtype], (M, F, dtype, delta)
    zero = got == 0
    assert np.array_equal(np.signbit(got[zero]), np.signbit(ref[zero])), "sign of a zero result"
    gate = y[:, F:]
    ovf = gate == round_half(np.float32(-65504.0), dtype)
    assert ovf.sum() >= 1 and (got[ovf] == 0).all() and np.array_equal(np.signbit(got[ovf]), ~np.signbit(y[:, :F][ovf]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_glu_swish_nan_positions(built_lib, dtype):
    """NaN exactly where a * silu(g) in fp32 on the CPU has it: NaN in either operand, an infinite a against a gate whose swish is 0
    (-65504, -100: exp overflows in fp32 there too) or exactly 0, an infinite gate."""
    K = _K()
    M, F = 3, 264
    y = _glu_input(M, F, dtype)
    a, g = y[:, :F], y[:, F:]
    a[0, 0] = np.inf; g[0, 0] = 0.0
    a[0, 9] = -np.inf; g[0, 9] = -65504.0
    a[0, 17] = np.inf; g[0, 17] = -100.0
    a[1, 3] = np.nan
    g[1, 200] = np.nan
    a[2, 263] = 0.0; g[2, 263] = np.inf
    a[2, 100] = 1.0; g[2, 100] = -np.inf
    a[2, 7] = np.inf; g[2, 7] = 2.0                 # +inf, no NaN
    y = round_half(np.concatenate([a, g], axis=1), dtype)
    want = torch.from_numpy(y[:, :F]) * torch.nn.functional.silu(torch.from_numpy(y[:, F:]))
    got = _np(K.glu_swish(_dev(y, _tdt(dtype))))
    assert np.array_equal(np.isnan(got), torch.isnan(want).numpy())
    assert int(np.isnan(got).sum()) == 7


@pytest.mark.parametrize("dtype", DTYPES)
def test_glu_swish_range_alarm(built_lib, dtype):
    """The f16 range alarm counts one lane per 8-element group that holds a result beyond +-65504 (a = g = 300 gives 90 000), however many of
    the group's elements do; a bf16 launch never counts; the counter adds to what it held; no counter at all is accepted (every other test)."""
    K = _K()
    M, F = 257, 264
    y = _glu_input(M, F, dtype)
    groups = [(0, 0), (0, 32), (5, 1), (200, 17), (256, 32)]            # (row, 8-element group of the row)
    for m, grp in groups:
        y[m, grp * 8 + 3] = 300.0; y[m, F + grp * 8 + 3] = 300.0
    y[5, 1 * 8 + 6] = -300.0; y[5, F + 1 * 8 + 6] = 300.0               # a second element of a group already counted
    y = round_half(y, dtype)
    ctr = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    got = _np(K.glu_swish(_dev(y, _tdt(dtype)), overflow=ctr))
    assert int(ctr.item()) == 1000 + (len(groups) if dtype == "f16" else 0)
    if dtype == "f16":      # saturated, not infinite
        assert got[0, 3] == 65504.0 and got[5, 14] == -65504.0 and np.isfinite(got).all()
    else:
        assert abs(got[0, 3] - 90000.0) <= 256.0


# ---- casts -------------------------------------------------------------------------------------------------------------------------------
def _f32_from_bits(bits):
    return np.array(bits, np.uint32).view(np.float32)


def _cast_specials(dtype):
    """+-0, subnormals of the target type (one exact, one on a tie, one below half the smallest), +-inf, NaN, and fp32 numbers on either
    side of the type's largest finite one."""
    if dtype == "f16":
        near = [65504.0, 65519.0, 65520.0, 65536.0, -65504.0, -65519.996, -65520.0, 1e9]
        sub = [2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -26, -(2.0 ** -24), 2.0 ** -15, 1023 * 2.0 ** -24]
        out = np.array([0.0, -0.0, np.inf, -np.inf, np.nan] + sub + near, np.float32)
    else:
        near = _f32_from_bits([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F0000, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF])
        sub = _f32_from_bits([0x00010000, 0x00018000, 0x00004000, 0x80010000, 0x007F0000, 0x00008001])
        out = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32), sub, near])
    return out


def _to_half_expected(x, dtype):
    """Round to nearest even like torch; an f16 destination saturates at +-65504 instead of producing inf (Half<_Float16>::from in
    common.h: a compare-and-select clamp in front of the conversion, NaN passes through), infinities included."""
    if dtype == "f16":
        with np.errstate(invalid="ignore"):
            x = np.where(x > 65504.0, np.float32(65504.0), np.where(x < -65504.0, np.float32(-65504.0), x)).astype(np.float32)
    return round_half(x, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * 1024 * 1024 + 4099])
def test_cast_to_half(built_lib, dtype, n):
    """fp32 -> operand type, bit for bit: the tail alone (n < 4), around one block of 4-element lanes, and past 4096 blocks x 256 threads x 4
    elements, where the grid-stride loop runs a second time."""
    K = _K()
    sp = _cast_specials(dtype)
    base = np.concatenate([sp, synth.normal("rows_cast", (65537 - sp.size,), 3.0)])
    x = np.roll(np.resize(base, max(n, 1)), 2 if n > 8 else 0)[:n]      # (short inputs start with the specials; long ones carry them in every period)
    if 0 < n <= 5:
        x = np.resize(np.roll(sp, -n), n)                               # another window of the specials per length
    got = K.to_half(_dev(x), dtype)
    assert got.shape == (n,) and got.dtype == _tdt(dtype)
    want = _to_half_expected(x, dtype)
    g = _np(got)
    assert np.array_equal(np.isnan(g), np.isnan(want))
    assert _same_f32(np.nan_to_num(g, nan=7.0), np.nan_to_num(want, nan=7.0)), (dtype, n, int((_f32_bits(g) != _f32_bits(want)).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_of_nothing(built_lib, dtype):
    """n = 0 succeeds and writes nothing, in both directions."""
    code = 0 if dtype == "f16" else 1
    src32, dsth = _full((8,), torch.float32, 1.0), _full((8,), _tdt(dtype))
    assert built_lib.avexhip_cast_f32_to_half(int(src32.data_ptr()), int(dsth.data_ptr()), 0, code, None) == 0
    dst32 = _full((8,), torch.float32)
    assert built_lib.avexhip_cast_half_to_f32(int(dsth.data_ptr()), int(dst32.data_ptr()), 0, code, None) == 0
    torch.cuda.synchronize()
    _untouched(dsth, 0, 0, "to_half")
    _untouched(dst32, 0, 0, "to_f32")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024 * 1024 + 4099])
def test_cast_to_f32(built_lib, dtype, n):
    """Operand type -> fp32 is exact, past 4096 blocks x 256 threads (the second trip of the grid-stride loop) too."""
    K = _K()
    sp = _to_half_expected(_cast_specials(dtype), dtype)
    base = np.concatenate([sp, round_half(synth.normal("rows_cast32", (65537 - sp.size,), 3.0), dtype)])
    x = np.resize(np.roll(base, -(n % 7)), n)
    h = _dev(x, _tdt(dtype))
    assert _same_f32(np.nan_to_num(_np(h), nan=7.0), np.nan_to_num(x, nan=7.0))      # the upload itself is exact
    got = K.to_f32(h).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(x))
    assert _same_f32(np.nan_to_num(got, nan=7.0), np.nan_to_num(x, nan=7.0)), (dtype, n)


# ---- zero_rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5])
def test_zero_rows(built_lib, M):
    """Masked rows (NaN before) become +0 in their first C columns; unmasked rows, the gap columns of every row and the guard row keep their
    bits.  No mask set, all set, alternating; the fp32 copy alone, the 16-bit copy alone (f16 and bf16 buffers), both."""
    K = _K()
    for Cc in (1, 255, 256, 257, 768):
        for mname, mask in (("none", np.zeros(M, np.uint8)), ("all", np.ones(M, np.uint8)), ("alt", (np.arange(M) % 2 == 0).astype(np.uint8) * 3)):
            for use32, useh in ((True, False), (False, True), (True, True)):
                hd = torch.float16 if Cc % 2 else torch.bfloat16
                x32 = _dev(synth.normal(f"rows_zr{Cc}", (M + 1, Cc + 3), 1.0))
                xh = _dev(synth.normal(f"rows_zrh{Cc}", (M + 1, Cc + 5), 1.0), hd)
                for m in range(M):
                    if mask[m]:
                        x32[m, :Cc] = float("nan"); xh[m, :Cc] = float("nan")
                b32, bh = _bits(x32).copy(), _bits(xh).copy()
                K.zero_rows(x32 if use32 else None, xh if useh else None, _dev(mask, torch.uint8), Cc)
                for m in range(M):
                    if mask[m]:
                        if use32:
                            b32[m, :Cc] = 0
                        if useh:
                            bh[m, :Cc] = 0
                assert np.array_equal(_bits(x32), b32), (M, Cc, mname, use32, useh, "fp32 copy")
                assert np.array_equal(_bits(xh), bh), (M, Cc, mname, use32, useh, "half copy")
    x32 = _full((M, 8), torch.float32)
    K.zero_rows(x32, None, None, 8)                     # no mask: nothing happens
    _untouched(x32, 0, 0, "pad = NULL")


# ---- row_sum_half / lnr_fold -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_sum_half(built_lib, dtype):
    """Row sums of a half matrix against the fp64 sum of the same rounded weights.  A lane adds ceil(K / 64) values in turn, the 64 lanes
    are combined in 6 butterfly levels; every addition rounds by at most 2^-24 of a partial sum, which never exceeds sum |w|:
    |err| <= (ceil(K / 64) + 6) * 2^-24 * sum |w|.  Row counts around the 4 rows of a workgroup, row lengths around the 64 lanes."""
    K = _K()
    for N in (1, 3, 4, 5, 768):
        for Kd in (1, 63, 64, 65, 768, 3072):
            w = round_half(synth.normal(f"rows_rs{N}_{Kd}", (N, Kd), 0.05) + np.float32(0.01), dtype)
            got = K.row_sum_half(_dev(w, _tdt(dtype))).cpu().numpy().astype(np.float64)
            bound = (math.ceil(Kd / 64) + 6) * 2.0 ** -24 * np.abs(w.astype(np.float64)).sum(axis=1)
            err = np.abs(got - R.row_sums(w))
            assert (err <= bound).all(), (dtype, N, Kd, float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("alpha", [1.0, 0.5, 1.7])
def test_lnr_fold(built_lib, alpha):
    """ga = gamma * alpha is one fp32 product: bit-exact.  bb = fma(alpha, beta, bias) is rounded once: within one fp32 ulp of fp64."""
    K = _K()
    for N in (1, 255, 256, 257, 768):
        gamma = (1.0 + synth.normal(f"rows_fg{N}", (N,), 0.2)).astype(np.float32)
        beta, bias = synth.normal(f"rows_fb{N}", (N,), 0.2), synth.normal(f"rows_fc{N}", (N,), 0.3)
        ga, bb = K.lnr_fold(_dev(gamma), _dev(beta), _dev(bias), alpha)
        assert _same_f32(ga.cpu().numpy(), gamma * np.float32(alpha)), (N, alpha)
        want = R.lnr_fold(gamma, beta, bias, alpha)[1]
        assert (np.abs(bb.cpu().numpy().astype(np.float64) - want) <= R.f32_ulp(want)).all(), (N, alpha)


# ---- bias_toeplitz -----------------------------------------------------------------------------------------------------------------------
def _saturation_distance(nb, md):
    """The handle's rule (beats_create): the first max_distance * 2^i at which both signs have reached their last bucket."""
    K = _K()
    last = nb // 2 - 1
    maxd = max(md, 1)
    while not (K.rel_bucket(-maxd, nb, md) == last and K.rel_bucket(maxd, nb, md) == nb // 2 + last):
        maxd *= 2
        assert maxd < 1 << 24
    return maxd


@pytest.mark.parametrize("nb,md,Ts", [(32, 64, (1, 2, 17, 70, 200)), (320, 800, (496,))])
def test_bias_toeplitz(built_lib, nb, md, Ts):
    """The [H, 2T - 1] bias rows from the bucket table and the host-made bucket LUT: equal to the same gather on the host and to the table
    built by asking avexhip_rel_bucket for every offset.  32 buckets / distance 64 saturate by 64, so 70 and 200 tokens reach the clamp."""
    K = _K()
    maxd = _saturation_distance(nb, md)
    assert maxd < 200 or nb == 320
    # the handle's distance, and the FIRST distance at which both signs sit in their last bucket: there the LUT's last entry differs from
    # the one before it, so a clamp that stops one short shows (at the handle's distance the two entries are equal)
    first = next(d for d in range(1, maxd + 1) if K.rel_bucket(-d, nb, md) == nb // 2 - 1 and K.rel_bucket(d, nb, md) == nb - 1)
    assert K.rel_bucket(first - 1, nb, md) != nb - 1
    for H in (1, 12):
        table = synth.normal(f"rows_tab{nb}_{H}", (nb, H), 0.5)
        for dist in (maxd, first):
            lut = K.bucket_lut(nb, md, dist)
            for T in Ts:
                got = K.bias_toeplitz(_dev(table), _dev(lut, torch.int32), dist, T).cpu().numpy()
                assert _same_f32(got, R.toeplitz(table, lut, dist, T)), (nb, md, H, T, dist, "host gather")
                assert _same_f32(got, _toeplitz_direct(table, T, nb, md)), (nb, md, H, T, dist, "bucket of every offset")


# ---- token_embed_ln ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,htol", [("f16", 6e-4), ("bf16", 4.8e-3)])
@pytest.mark.parametrize("Cc", [64, 128, 1024])
def test_token_embed_ln_shapes(built_lib, dtype, htol, Cc):
    """test_gpu_eat.py::test_token_embed_ln_matches_oracle (768 wide, 512 patches, f16) at one, two and sixteen values per lane, with
    fewer rows than a workgroup holds and with a workgroup that spans two clips, in both operand types.  Same oracle (O.layer_norm), same
    bars: rel-L2 5e-6 for the fp32 rows, 6e-4 for f16 rows; bf16 rounds with 3 mantissa bits less: 8 x 6e-4."""
    K = _K()
    for Tp in (1, 3, 5):
        for B in (1, 2):
            pe = round_half(synth.normal(f"rows_te{Cc}_{Tp}_{B}", (B * Tp, Cc), 1.0), dtype)
            pos = synth.normal(f"rows_tepos{Cc}", (Tp, Cc), 0.5)
            cls = synth.normal("rows_tecls", (Cc,), 0.5)
            w = (1.0 + synth.normal("rows_tew", (Cc,), 0.1)).astype(np.float32)
            b = synth.normal("rows_teb", (Cc,), 0.1)
            outh, outf = K.token_embed_ln(_dev(pe, _tdt(dtype)), _dev(pos), _dev(cls), _dev(w), _dev(b), 1e-6, B, want_f32=True)
            x = pe.reshape(B, Tp, Cc) + pos[None]
            x = np.concatenate([np.broadcast_to(cls, (B, 1, Cc)), x], 1)
            ref = O.layer_norm(x.astype(np.float32), w, b, 1e-6).reshape(B * (Tp + 1), Cc)
            assert outf.shape == ref.shape and outh.dtype == _tdt(dtype)
            assert rel_l2(outf.cpu().numpy(), ref) < 5e-6, (dtype, Cc, Tp, B)
            assert rel_l2(_np(outh), ref) < htol, (dtype, Cc, Tp, B)
            assert _same_f32(_np(outh), round_half(outf.cpu().numpy(), dtype)), (dtype, Cc, Tp, B, "half rows are not the rounding of the fp32 rows")
