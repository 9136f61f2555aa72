"""The GEMM options the encoder handles use -- row_zero, half_scale, n_store, a_scale, post_ln_*, activation codes 3-5, leading
dimensions, and the skinny kernel's remaining instantiations and trips -- one kernel form at a time through avexhip_gemm (ABI 18).

Most statements are bit-exact: they follow from the kernels' arithmetic (the library is built with -ffp-contract=off, so an expression
written once in common.h gives the same bits in every kernel that inlines it).  Where only fp64 can judge, the measure is the rel-L2 of
each output ROW (tests/_gemm_ref.py): 1e-5 for fp32 rows, 2e-3 (f16) / 1.5e-2 (bf16) for rows in the operand type."""
import pytest
import torch

import _gemm_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SENT = -1984.0          # exact in f16, bf16 and fp32: a buffer filled with it shows every element a kernel wrote
ALPHA = 2.2133638


def _K():
    from avex_amd import kernels
    return kernels


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, scale, seed, dtype=torch.float32):
    return (torch.randn(shape, generator=_gen(seed), device="cuda") * scale).to(dtype)


def _bits(x):
    x = x.contiguous()
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _assert_same(r, ref, keys, what):
    for k in keys:
        assert _same(r[k], ref[k]), (what, k, int((_bits(r[k]) != _bits(ref[k])).sum()))


def _assert_rows(got, want, tol, what):
    err, row = R.worst_row(got, want)
    assert err < tol, (what, f"row {row}: rel-L2 {err:.3e} >= {tol:.1e}")


# the kernel forms of avx::gemm: 128-tile register staging, 128-tile LDS-DMA, 256-tile streaming (generic epilogue whenever an fp32 / raw
# output, a mask, a scale or an activation code above 2 is asked for), split-K (K >= 1024 with a workspace), skinny
FORMS = {"v1": dict(variant=1), "v3": dict(variant=3), "v5": dict(variant=5), "splitk": dict(variant=3, splitk=True), "v7": dict(variant=7)}


def _operands(dtype, M, N, Kd, seed):
    td = R.tdt(dtype)
    return _randn((M, Kd), 1.0, seed, td), _randn((N, Kd), 0.05, seed + 1, td), _randn((N,), 0.3, seed + 2)


# ---- row_zero ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["v1", "v3", "v5", "splitk", "splitk_ln"])
def test_row_zero(built_lib, dtype, form):
    """Masked rows take 0 in place of acc + bias in every kernel form that knows the mask: exactly 0.0 in the raw tap, and in every output
    when there is no residual; with a residual they come out as act(resid * alpha) -- the product is zeroed BEFORE the residual is added
    (the only caller, the projection behind the patch embedding, has no residual).  Unmasked rows do not notice the mask."""
    K = _K()
    td = R.tdt(dtype)
    M, N = 130, 256
    Kd = 1024 if form.startswith("splitk") else 128
    a, w, bias = _operands(dtype, M, N, Kd, 100)
    mask = torch.rand(M, generator=_gen(7), device="cuda") < 1.0 / 3.0
    mask[[0, 15, 16, 127, 128, 129]] = True
    mask[[1, 14, 17, 126]] = False
    kw = dict(FORMS["splitk" if form == "splitk_ln" else form], bias=bias, out_f32=True, out_half=True, out_raw=True)
    keys = ["f32", "half", "raw"]
    act = 3
    if form == "splitk_ln":
        gamma, beta = 1.0 + _randn((N,), 0.2, 8), _randn((N,), 0.2, 9)
        kw.update(post_ln_w=gamma, post_ln_b=beta, post_ln_out_half=True)
        keys += ["ln_f32", "ln_half"]
        act = 0          # (post_ln takes no activation)
    plain = K.gemm(a, w, **kw)
    r = K.gemm(a, w, row_zero=mask, **kw)
    for k in ("f32", "half", "raw"):
        assert bool((r[k][mask] == 0).all()), (k, "masked rows must be exactly zero")
    assert bool((plain["raw"][mask] != 0).any())
    for k in keys:
        assert _same(r[k][~mask], plain[k][~mask]), (k, "unmasked rows")
    if form == "splitk_ln":      # LayerNorm of a zero row: (0 - 0) * rstd * w + b = b, exactly
        assert _same(r["ln_f32"][mask], beta.expand(M, N)[mask]) and _same(r["ln_half"][mask], beta.to(td).expand(M, N)[mask])
    al = torch.tensor(ALPHA, dtype=torch.float32, device="cuda")
    for rk, res in (("resid", _randn((M, N), 1.0, 11)), ("resid_half", _randn((M, N), 1.0, 12, td))):
        kwr = dict(kw, alpha=ALPHA, act=act, **{rk: res})
        plain = K.gemm(a, w, **kwr)
        r = K.gemm(a, w, row_zero=mask, **kwr)
        assert bool((r["raw"][mask] == 0).all()), (rk, "raw tap of masked rows")
        want = res.float() * al          # resid * alpha + 0: one fp32 rounding, as a multiply-add or as a fused one
        if act == 3:
            want = torch.relu(want)
        assert _same(r["f32"][mask], want[mask]), (rk, "masked rows = act(resid * alpha)")
        assert _same(r["half"][mask], want.to(td)[mask]), (rk, "masked rows, operand type")
        for k in keys:
            assert _same(r[k][~mask], plain[k][~mask]), (rk, k, "unmasked rows")


# ---- half_scale --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shift", [1, 4, 8])
def test_half_scale(built_lib, dtype, shift):
    """out_half = round(value * 2^-shift) while out_f32 and out_raw stay unscaled: the scale is a power of two, so value * scale is exact in
    fp32 and the half output is round_half(f32 * scale) bit for bit.  The streaming kernel's fast epilogues do not know the scale: the
    planner must fall back to the generic one, which gives the 128-tile kernel's bits."""
    K = _K()
    td = R.tdt(dtype)
    scale = 2.0 ** -shift
    M, N = 130, 256
    out = {}
    for form in ("v1", "v3", "v5", "splitk"):
        a, w, bias = _operands(dtype, M, N, 1024 if form == "splitk" else 128, 200)
        kw = dict(FORMS[form], bias=bias, out_f32=True, out_half=True, out_raw=True)
        plain = K.gemm(a, w, **kw)
        r = out[form] = K.gemm(a, w, half_scale=scale, **kw)
        assert _same(r["half"], (r["f32"] * scale).to(td)), form
        assert not _same(r["half"], plain["half"]), form
        _assert_same(r, plain, ("f32", "raw"), form)
        # the half-only launch (what fc1 of the range ladder is): the streaming kernel would take its fast epilogue without the scale
        rh = K.gemm(a, w, half_scale=scale, **dict(kw, out_f32=False, out_raw=False))
        assert _same(rh["half"], r["half"]), (form, "half output alone")
    _assert_same(out["v5"], out["v3"], ("f32", "half", "raw"), "variant 5 against variant 3")
    _assert_same(out["v1"], out["v3"], ("f32", "half", "raw"), "variant 1 against variant 3")


def test_half_scale_refusals(built_lib):
    K = _K()
    from avex_amd._capi import AvexHipError
    a, w, bias = _operands("f16", 128, 256, 128, 210)
    ones = torch.ones(256, device="cuda")
    for what, kw in (("stats_out", dict(stats_out=True)), ("pool_rows", dict(pool_rows=64)), ("variant 7", dict(variant=7)),
                     ("post_ln", dict(splitk=True, post_ln_w=ones, post_ln_b=ones)), ("negative", dict(half_scale=-0.5))):
        with pytest.raises(AvexHipError):
            K.gemm(a, w, bias=bias, out_f32=False, out_half=True, **dict(dict(half_scale=0.5), **kw))
        if "half_scale" not in kw:      # ... and it is the scale that is refused: the same launch without it runs
            assert K.gemm(a, w, bias=bias, out_f32=False, out_half=True, **kw)["half"].shape[1] == 256, what
    assert K.gemm(a, w, bias=bias, out_f32=False, out_half=True, half_scale=1.0, variant=7)["half"].shape == (128, 256)      # 1 is "off"


# ---- n_store -----------------------------------------------------------------------------------------------------------------------------
def _n_store_case(K, dtype, form, M, N, Kd, ns, seed):
    td = R.tdt(dtype)
    a, w, bias = _operands(dtype, M, N, Kd, seed)
    res_full = _randn((M, N), 1.0, seed + 3, td)
    res = res_full[:, :ns].contiguous()          # the residual exists ns columns wide only
    skinny = form == "v7"
    keys = ["half"] if skinny else ["f32", "half", "raw"]
    kw = dict(FORMS[form], bias=bias, alpha=0.5, silu=True, out_f32=not skinny, out_half=True, out_raw=not skinny)
    full = K.gemm(a, w, resid_half=res_full, **kw)
    what = (form, M, N, Kd, ns)
    # rows N wide: the columns from n_store on are never written
    r = K.gemm(a, w, resid_half=res, n_store=ns, ld_out=N, sentinel=SENT, **kw)
    for k in keys:
        buf = r[k + "_buf"]
        assert buf.shape == (M, N)
        assert bool((buf[:, ns:] == SENT).all()), (what, k, "columns >= n_store were written")
        assert _same(buf[:, :ns], full[k][:, :ns]), (what, k, "columns < n_store")
    # rows n_store wide, a guard behind the last one
    r = K.gemm(a, w, resid_half=res, n_store=ns, ld_out=ns, guard_rows=2, sentinel=SENT, **kw)
    for k in keys:
        buf = r[k + "_buf"]
        assert buf.shape == (M + 2, ns) and r[k].shape == (M, ns)
        assert _same(r[k], full[k][:, :ns]), (what, k, "rows n_store wide")
        assert bool((buf[M:] == SENT).all()), (what, k, "guard rows were written")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["v1", "v3", "splitk"])
def test_n_store_128_tile(built_lib, dtype, form):
    """Narrow outputs of the 128-tile kernels (EfficientNet's channel counts below the tile width): the product is computed N wide, rows
    of the outputs and the residual exist n_store wide.  Nothing from column n_store on is written, in rows N wide (sentinel columns) or
    n_store wide (the next row, and a guard behind the last); the stored columns are those of the full-width launch."""
    K = _K()
    Kd = 1024 if form == "splitk" else 128
    for M in (1, 130):
        for N, ns in ((128, 4), (128, 100), (128, 124), (256, 132)):
            _n_store_case(K, dtype, form, M, N, Kd, ns, 300 + ns)


@pytest.mark.parametrize("dtype", DTYPES)
def test_n_store_skinny(built_lib, dtype):
    """... and of the skinny kernel, whose lanes store runs of 16 columns (N = 64, 128) or 8 (N = 96: the G = 2 form)."""
    K = _K()
    for M in (1, 130):
        for N, Kd, ns in ((64, 32, 16), (64, 32, 48), (96, 64, 16), (128, 64, 16), (128, 64, 112)):
            _n_store_case(K, dtype, "v7", M, N, Kd, ns, 340 + ns)


# ---- a_scale -----------------------------------------------------------------------------------------------------------------------------
def _scales(M, rows, Kd, seed):
    """Sigmoid-range scales, one row per clip of `rows` rows, a_scale_ld = Kd + 8 (NaN beside the K columns a kernel may read)."""
    clips = (M + rows - 1) // rows
    s = torch.full((clips, Kd + 8), float("nan"), device="cuda")
    s[:, :Kd] = torch.sigmoid(_randn((clips, Kd), 1.5, seed))
    return s


A_SCALE_M = 3 * 50 + 7      # no multiple of rows * 32 for rows = 1, 49, 50: the last clip is partial and the clamped tail rows read its scales


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Kd", [(32, 96), (64, 32), (128, 160), (256, 128), (96, 64)])
def test_a_scale_skinny(built_lib, dtype, N, Kd):
    """The per-(clip, input channel) rescale of the A rows on their way into the skinny kernel's MFMA operands: the fp32 product rounded to
    the operand type, so the launch equals the unscaled launch on (a.float() * s[row // rows]).to(half), bit for bit -- with clips of 1, 49
    and 50 rows the 16-row operand groups straddle clips.  The RAW form (N = 32 / 64 / 128 / 256) writes acc + bias as well."""
    K = _K()
    from avex_amd._capi import AvexHipError
    td = R.tdt(dtype)
    M = A_SCALE_M
    a, w, bias = _operands(dtype, M, N, Kd, 400)
    res = _randn((M, N), 1.0, 404, td)
    for rows in (1, 49, 50):
        s = _scales(M, rows, Kd, 410 + rows)
        sa = R.scaled_rows(a, s, rows)
        assert not _same(sa, a)
        for kw in (dict(bias=bias), dict(bias=bias, resid_half=res, alpha=0.5, silu=True)):
            kw = dict(kw, out_f32=False, out_half=True, variant=7)
            want = K.gemm(sa, w, **kw)
            got = K.gemm(a, w, a_scale=s, a_scale_rows=rows, **kw)
            assert _same(got["half"], want["half"]), (rows, sorted(kw))
            if N % 128 == 0 and Kd % 64 == 0:      # (256, 128): the register-staged 128-tile kernel takes the shape and the scale too
                assert _same(K.gemm(a, w, a_scale=s, a_scale_rows=rows, **dict(kw, variant=1))["half"], got["half"]), (rows, "variant 1")
            if N == 96:
                with pytest.raises(AvexHipError):
                    K.gemm(a, w, a_scale=s, a_scale_rows=rows, out_raw=True, **kw)
                continue
            raw = K.gemm(a, w, a_scale=s, a_scale_rows=rows, out_raw=True, **kw)
            assert _same(raw["half"], want["half"]), (rows, "half output of the RAW form")
            ref = R.gemm_ref(a, w, dtype, bias=bias, a_scale=s, a_scale_rows=rows)
            _assert_rows(raw["raw"], ref["raw"], R.F32_ROW_TOL, (rows, "raw tap"))
            if "resid_half" not in kw:       # no residual, no activation: the half output is the rounded tap
                assert _same(raw["half"], raw["raw"].to(td)), (rows, "half = round(raw)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Kd", [64, 192])
def test_a_scale_variant_1(built_lib, dtype, Kd):
    """The same rescale in the register-staged 128-tile kernel (EfficientNet's squeeze-excitation fold where the skinny kernel has no
    shape), against itself on pre-scaled rows and, at K = 64, against the skinny kernel."""
    K = _K()
    td = R.tdt(dtype)
    M, N = A_SCALE_M, 128
    a, w, bias = _operands(dtype, M, N, Kd, 450)
    res = _randn((M, N), 1.0, 454, td)
    for rows in (1, 49, 50):
        s = _scales(M, rows, Kd, 460 + rows)
        sa = R.scaled_rows(a, s, rows)
        kw = dict(bias=bias, resid_half=res, alpha=0.5, silu=True, out_f32=True, out_half=True, out_raw=True, variant=1)
        want = K.gemm(sa, w, **kw)
        got = K.gemm(a, w, a_scale=s, a_scale_rows=rows, **kw)
        _assert_same(got, want, ("f32", "half", "raw"), rows)
        _assert_rows(got["raw"], R.gemm_ref(a, w, dtype, bias=bias, a_scale=s, a_scale_rows=rows)["raw"], R.F32_ROW_TOL, (rows, "raw tap"))
        if Kd == 64:
            r7 = K.gemm(a, w, a_scale=s, a_scale_rows=rows, **dict(kw, variant=7, out_f32=False))
            _assert_same(r7, got, ("half", "raw"), (rows, "variant 7 against variant 1"))


def test_a_scale_refusals(built_lib):
    K = _K()
    from avex_amd._capi import AvexHipError
    a, w, bias = _operands("f16", 64, 128, 64, 470)
    s = _scales(64, 16, 64, 471)
    for kw in (dict(variant=3), dict(variant=5), dict(variant=0)):
        with pytest.raises(AvexHipError):
            K.gemm(a, w, bias=bias, a_scale=s, a_scale_rows=16, out_f32=False, out_half=True, **kw)
    with pytest.raises(AvexHipError):      # a_scale_ld < K
        K.gemm(a, w, bias=bias, a_scale=s[:, :32].contiguous(), a_scale_rows=16, out_f32=False, out_half=True, variant=7)


# ---- post_ln -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [256, 512, 768, 1024])
def test_post_ln(built_lib, dtype, N):
    """LayerNorm of the finished rows in the split-K epilogue (one wave per row, one to four 256-column chunks per lane, four rows per
    workgroup).  y itself (fp32, half, raw tap) is what the launch without post_ln writes, bit for bit.  The LayerNorm outputs are judged
    per row against the fp64 LayerNorm of the y THIS launch wrote (the half y with post_ln_round, the fp32 y without): avexhip_layernorm
    sums a row in another order (a half-wave per row, or squares added pairwise), so the two kernels do not give the same bits."""
    K = _K()
    td = R.tdt(dtype)
    gamma, beta = 1.0 + _randn((N,), 0.2, 500), _randn((N,), 0.2, 501)
    n_same = n_rows = 0
    for M in (1, 5, 130):
        res = _randn((M, N), 1.0, 510 + M, td)
        mask = torch.arange(M, device="cuda") % 3 == 0
        for Kd in (64, 1024, 3072):
            a, w, bias = _operands(dtype, M, N, Kd, 520 + Kd)
            w = (w.float() * (8.0 / Kd ** 0.5)).to(td)
            for rnd in (0, 1):
                for extras in (False, True):
                    kw = dict(bias=bias, out_f32=True, out_half=True, variant=3, splitk=True)
                    if extras:
                        kw.update(resid_half=res, alpha=ALPHA, out_raw=True, row_zero=mask)
                    what = (M, Kd, rnd, extras)
                    plain = K.gemm(a, w, **kw)
                    r = K.gemm(a, w, post_ln_w=gamma, post_ln_b=beta, post_ln_eps=1e-5, post_ln_round=rnd, post_ln_out_half=True, **kw)
                    _assert_same(r, plain, [k for k in ("f32", "half", "raw") if k in plain], what)
                    y = r["half"] if rnd else r["f32"]
                    want = R.layer_norm(y.double(), gamma, beta, 1e-5)
                    _assert_rows(r["ln_f32"], want, R.F32_ROW_TOL, (what, "ln_f32"))
                    _assert_rows(r["ln_half"], want, R.F16_ROW_TOL[dtype], (what, "ln_half"))
                    assert _same(r["ln_half"], r["ln_f32"].to(td)), (what, "the half copy is the rounded fp32 one")
                    l32, _ = K.layernorm(y, gamma, beta, 1e-5, half_dtype=dtype, want_half=False)
                    n_same += int((_bits(l32) == _bits(r["ln_f32"])).all(dim=1).sum()); n_rows += M
                    _assert_rows(l32, want, R.F32_ROW_TOL, (what, "avexhip_layernorm"))
    print(f"post_ln N={N} {dtype}: {n_same} of {n_rows} rows have avexhip_layernorm's bits")


def test_post_ln_refusals(built_lib):
    K = _K()
    from avex_amd._capi import AvexHipError

    def launch(N, **kw):
        a, w, bias = _operands("f16", 5, N, 128, 560)
        ones = torch.ones(N, device="cuda")
        return K.gemm(a, w, **dict(dict(bias=bias, out_f32=True, variant=3, splitk=True, post_ln_w=ones, post_ln_b=ones), **kw))

    assert launch(256)["ln_f32"].shape == (5, 256)
    for kw in (dict(N=1280), dict(N=384), dict(N=256, act=3), dict(N=256, gelu=True), dict(N=256, n_store=128), dict(N=256, splitk=False)):
        with pytest.raises(AvexHipError):
            launch(**kw)


# ---- activation codes 3, 4, 5 ------------------------------------------------------------------------------------------------------------
# The largest |kernel - fp64 formula of the launch's own raw tap| over the inputs below, as measured on an MI355X (gfx950): tanh-form
# GELU 4.295e-7 (f16 inputs; 4.090e-7 bf16), tanh 2.023e-7 (1.830e-7), the same in every kernel form.  The tests assert four times that --
# headroom over the one input set it was measured on: 1.7e-6 and 8.1e-7, far below the 1e-5 an fp32 output may be off.
ACT_MEASURED_ABS = {4: 4.295e-7, 5: 2.023e-7}
ACT_CEILING = 1e-5


def _act_inputs(dtype, Kd):
    """raw[m, n] = a[m, n % 128] + bias[n] exactly (W selects one column; bias is 0 for the first 128 columns): the pre-activations span
    [-12, 12] with exact 0, +-12 and the magnitudes where tanh_fast saturates among them; Kd > 128 pads the contraction with zeros."""
    td = R.tdt(dtype)
    M, N = 130, 256
    a = torch.linspace(-12.0, 12.0, M * 128, device="cuda")[torch.randperm(M * 128, generator=_gen(600), device="cuda")].reshape(M, 128)
    a[0, :8] = torch.tensor([0.0, 12.0, -12.0, 9.0, -9.0, 10.5, -10.5, -0.0], device="cuda")
    w = torch.zeros((N, Kd), device="cuda")
    w[torch.arange(N), torch.arange(N) % 128] = 1.0
    bias = torch.cat([torch.zeros(128, device="cuda"), _randn((128,), 0.05, 601)])
    ap = torch.zeros((M, Kd), device="cuda")
    ap[:, :128] = a
    return ap.to(td), w.to(td), bias


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [3, 4, 5])
def test_activation_codes(built_lib, dtype, act):
    """ReLU, tanh-form GELU and tanh (act4_any) in every kernel that applies them -- variants 1 and 3, the split-K epilogue, the streaming
    kernel's generic epilogue (where the planner sends these codes) and the skinny kernel -- on each launch's own raw tap.  ReLU is exact.
    The other two are built on the hardware's exp2 and reciprocal approximations: their deviation from the fp64 formula is bounded by four
    times what was measured on the GPU.  All forms give each other's bits."""
    K = _K()
    td = R.tdt(dtype)
    out = {}
    for form in ("v1", "v3", "v5", "splitk"):
        a, w, bias = _act_inputs(dtype, 1024 if form == "splitk" else 128)
        r = out[form] = K.gemm(a, w, bias=bias, act=act, out_f32=True, out_half=True, out_raw=True, **FORMS[form])
        raw = r["raw"]
        assert float(raw.min()) < -11.9 and float(raw.max()) > 11.9 and bool((raw == 0).any())
        assert _same(raw, a[:, :128].float().repeat(1, 2) + bias), (form, "the raw tap is a + bias exactly")
        want = R.activation(raw.double(), act)
        if act == 3:
            assert _same(r["f32"], torch.clamp_min(raw, 0.0)), form
        else:
            dev = float((r["f32"].double() - want).abs().max())
            print(f"act {act} {form} {dtype}: max |kernel - fp64| = {dev:.3e}")
            bound = 4.0 * ACT_MEASURED_ABS[act]
            assert bound <= ACT_CEILING
            assert dev <= bound, (form, dev, bound)
        assert _same(r["half"], r["f32"].to(td)), (form, "the half output is the rounded fp32 one")
    a, w, bias = _act_inputs(dtype, 128)
    # bias + activation + half output alone is the streaming kernel's fast epilogue for codes 1 and 2; these codes must take the generic one
    r5 = K.gemm(a, w, bias=bias, act=act, out_f32=False, out_half=True, variant=5)
    assert _same(r5["half"], out["v5"]["half"]), "variant 5, half output alone"
    ones = torch.ones((1, 128), device="cuda")      # a scale of 1.0 leaves the rows as they are and opens the skinny kernel's raw tap
    r7 = K.gemm(a, w, bias=bias, act=act, out_f32=False, out_half=True, out_raw=True, a_scale=ones, a_scale_rows=130, variant=7)
    for form in ("v1", "v5", "splitk"):
        _assert_same(out[form], out["v3"], ("f32", "half", "raw"), (form, "against variant 3"))
    _assert_same(r7, out["v3"], ("half", "raw"), "variant 7 against variant 3")


# ---- the skinny kernel: remaining instantiations, short and long row counts -----------------------------------------------------------------
SKINNY_MISSING = [(32, 32), (32, 64), (32, 96), (32, 128), (32, 160), (32, 256), (96, 32), (160, 32), (256, 32)]


def _skinny_cases(dtype, M, N, Kd, seed, rows):
    td = R.tdt(dtype)
    a, w, bias = _operands(dtype, M, N, Kd, seed)
    w = (w.float() * 2.0).to(td)
    res = _randn((M, N), 1.0, seed + 3, td)
    s = _scales(M, rows, Kd, seed + 4)
    return a, w, [("plain", dict(), dict()),
                  ("bias + residual + SiLU", dict(bias=bias, resid_half=res, alpha=0.5, silu=True), dict(bias=bias, resid=res, alpha=0.5, act=2)),
                  ("a_scale", dict(bias=bias, a_scale=s, a_scale_rows=rows), dict(bias=bias, a_scale=s, a_scale_rows=rows))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Kd", SKINNY_MISSING)
def test_skinny_instantiations_short_rows(built_lib, dtype, N, Kd):
    """The nine (N, K) of AVX_SKINNY_SHAPES that test_gemm_skinny_streaming does not reach (N = 32, and K = 32 with N = 96 / 160 / 256), in
    the plain and the SCALE form, at row counts below and around one workgroup's 128 rows: every row against fp64."""
    K = _K()
    for M in (1, 31, 33, 127, 129):
        a, w, cases = _skinny_cases(dtype, M, N, Kd, 700 + M, 7)
        for name, kw, ref_kw in cases:
            got = K.gemm(a, w, out_f32=False, out_half=True, variant=7, **kw)["half"]
            assert got.shape == (M, N)
            _assert_rows(got, R.gemm_ref(a, w, dtype, **ref_kw)["half"], R.F16_ROW_TOL[dtype], (M, name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Kd,per_cu", [(128, 64, 4), (128, 256, 2)])
def test_skinny_long_rows_make_several_trips(built_lib, dtype, N, Kd, per_cu):
    """Twice the planner's grid of 128-row blocks and a few rows more: every workgroup makes two trips and the first ones three, so the
    prefetch of the next trip's rows (K <= 128), its clamp at the last trip and the mode switch in front of the later trips' MFMAs run.
    Against the 128-tile kernel's bits, and against fp64 on the first, last and 2 000 evenly spaced rows and those around every trip boundary."""
    K = _K()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    grid = n_cu * per_cu
    M = 128 * grid * 2 + 77
    a, w, cases = _skinny_cases(dtype, M, N, Kd, 800 + Kd, 196)      # clips of 14 x 14 rows: no multiple of 16, operand groups straddle clips on every trip
    idx = torch.linspace(0, M - 1, 2000, device="cuda").long()
    edges = torch.tensor([t * 128 * grid + d for t in (1, 2) for d in range(-2, 3)] + [0, M - 1], device="cuda")
    idx = torch.unique(torch.cat([idx, edges]))
    for name, kw, ref_kw in cases:
        got = K.gemm(a, w, out_f32=False, out_half=True, variant=7, **kw)["half"]
        if "a_scale" in kw:
            a3, kw3 = R.scaled_rows(a, kw["a_scale"], kw["a_scale_rows"]), dict(bias=kw["bias"])
            assert _same(K.gemm(a3, w, out_f32=False, out_half=True, variant=7, **kw3)["half"], got), (name, "against pre-scaled rows")
        else:
            a3, kw3 = a, kw
        assert _same(K.gemm(a3, w, out_f32=False, out_half=True, variant=3, **kw3)["half"], got), (name, "against variant 3")
        if "resid" in ref_kw:
            ref_kw = dict(ref_kw, resid=ref_kw["resid"][idx])
        if "a_scale" in ref_kw:      # the sampled rows keep their own clips' scales
            ref = R.gemm_ref(R.scaled_rows(a, kw["a_scale"], kw["a_scale_rows"])[idx], w, dtype, bias=ref_kw["bias"])
        else:
            ref = R.gemm_ref(a[idx], w, dtype, **ref_kw)
        _assert_rows(got[idx], ref["half"], R.F16_ROW_TOL[dtype], (name, "sampled rows"))


# ---- leading dimensions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["v1", "v3", "v5", "v7", "splitk"])
def test_leading_dimensions(built_lib, dtype, form):
    """Outputs and residual as column slices of wider buffers (ld = N + 64) and weight rows K + 8 apart, as the handles lay them out:
    the values of the contiguous launch, and nothing written beside them."""
    K = _K()
    td = R.tdt(dtype)
    M, N = 130, 256
    a, w, bias = _operands(dtype, M, N, 1024 if form == "splitk" else 128, 900)
    res = _randn((M, N), 1.0, 903, td)
    skinny = form == "v7"
    keys = ["half"] if skinny else ["f32", "half", "raw"]
    kw = dict(FORMS[form], bias=bias, resid_half=res, alpha=0.5, silu=True, out_f32=not skinny, out_half=True, out_raw=not skinny)
    ref = K.gemm(a, w, **kw)
    r = K.gemm(a, w, ld_out=N + 64, ldw=a.shape[1] + 8, guard_rows=1, sentinel=SENT, **kw)
    for k in keys:
        buf = r[k + "_buf"]
        assert buf.shape == (M + 1, N + 64) and r[k].shape == (M, N)
        assert _same(r[k], ref[k]), (form, k)
        assert bool((buf[:, N:] == SENT).all()) and bool((buf[M:] == SENT).all()), (form, k, "padding was written")
