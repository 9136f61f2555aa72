"""tests/_gemm_ref.py (the fp64 restatement of avexhip_gemm's epilogue that test_gpu_gemm_args.py compares the kernels with) against
torch.nn.functional in fp64, on tiny shapes: Linear + activation + LayerNorm, and each option's place in the order.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R

DTYPES = ["f16", "bf16"]


def _case(dtype, M=7, N=12, K=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    td = R.tdt(dtype)
    a = torch.randn(M, K, generator=g).to(td)
    w = (0.3 * torch.randn(N, K, generator=g)).to(td)
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    return a, w, bias, resid


TORCH_ACT = {0: lambda x: x, 1: F.gelu, 2: F.silu, 3: F.relu, 4: lambda x: F.gelu(x, approximate="tanh"), 5: torch.tanh}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", sorted(TORCH_ACT))
def test_linear_activation_layernorm_match_torch(dtype, act):
    a, w, bias, resid = _case(dtype)
    gamma, beta = 1.0 + 0.1 * torch.randn(12, generator=torch.Generator().manual_seed(1)), torch.linspace(-1, 1, 12)
    r = R.gemm_ref(a, w, dtype, bias=bias, resid=resid, alpha=0.75, act=act, post_ln_w=gamma, post_ln_b=beta, post_ln_eps=1e-5)
    lin = F.linear(a.double(), w.double(), bias.double())
    assert torch.allclose(r["raw"], lin, rtol=0, atol=1e-14)
    want = TORCH_ACT[act](resid.double() * 0.75 + lin)
    assert torch.allclose(r["f32"], want, rtol=0, atol=1e-13), act
    assert torch.equal(r["half"], want.float().to(R.tdt(dtype)).double())
    ln = F.layer_norm(want, (12,), gamma.double(), beta.double(), 1e-5)
    assert torch.allclose(r["ln_f32"], ln, rtol=0, atol=1e-12)
    # post_ln_round: the LayerNorm reads the rows as the operand type holds them
    rr = R.gemm_ref(a, w, dtype, bias=bias, resid=resid, alpha=0.75, act=act, post_ln_w=gamma, post_ln_b=beta, post_ln_round=1)
    assert torch.allclose(rr["ln_f32"], F.layer_norm(r["half"], (12,), gamma.double(), beta.double(), 1e-5), rtol=0, atol=1e-12)
    assert not torch.equal(rr["ln_f32"], r["ln_f32"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_zero_comes_before_the_tap_and_the_residual(dtype):
    a, w, bias, resid = _case(dtype)
    mask = torch.tensor([1, 0, 0, 1, 0, 0, 1], dtype=torch.uint8)
    r = R.gemm_ref(a, w, dtype, bias=bias, row_zero=mask, resid=resid, alpha=2.0, act=3)
    full = R.gemm_ref(a, w, dtype, bias=bias, resid=resid, alpha=2.0, act=3)
    m = mask.bool()
    assert (r["raw"][m] == 0).all() and torch.equal(r["raw"][~m], full["raw"][~m])
    assert torch.equal(r["f32"][m], F.relu(resid.double()[m] * 2.0)) and torch.equal(r["f32"][~m], full["f32"][~m])
    assert (R.gemm_ref(a, w, dtype, bias=bias, row_zero=mask, act=5)["half"][m] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_half_scale_touches_the_half_output_only(dtype):
    a, w, bias, _ = _case(dtype)
    r0 = R.gemm_ref(a, w, dtype, bias=bias)
    for s in (0.5, 2.0 ** -4, 2.0 ** -8):
        r = R.gemm_ref(a, w, dtype, bias=bias, half_scale=s)
        assert torch.equal(r["f32"], r0["f32"]) and torch.equal(r["raw"], r0["raw"])
        assert torch.equal(r["half"], (r0["f32"] * s).float().to(R.tdt(dtype)).double())
    assert torch.equal(R.gemm_ref(a, w, dtype, bias=bias, half_scale=1.0)["half"], r0["half"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_n_store_keeps_the_leading_columns(dtype):
    a, w, bias, resid = _case(dtype)
    full = R.gemm_ref(a, w, dtype, bias=bias, resid=resid, act=2)
    r = R.gemm_ref(a, w, dtype, bias=bias, resid=resid[:, :4].contiguous(), act=2, n_store=4)
    for k in ("raw", "f32", "half"):
        assert r[k].shape == (7, 4) and torch.equal(r[k], full[k][:, :4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_scale_rounds_the_scaled_rows_to_the_operand_type(dtype):
    a, w, bias, _ = _case(dtype, M=11)
    scale = torch.rand(4, 12, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05      # ld 12 > K = 8, 3 rows per clip, last clip partial
    sa = R.scaled_rows(a, scale, 3)
    assert sa.dtype == a.dtype
    for m in range(11):
        assert torch.equal(sa[m], (a[m].float() * scale[m // 3, :8]).to(a.dtype))
    r = R.gemm_ref(a, w, dtype, bias=bias, a_scale=scale, a_scale_rows=3)
    assert torch.allclose(r["f32"], F.linear(sa.double(), w.double(), bias.double()), rtol=0, atol=1e-14)
    assert not torch.allclose(r["f32"], F.linear(a.double() * scale[torch.arange(11) // 3, :8].double(), w.double(), bias.double()), rtol=0, atol=1e-6)


def test_row_errors_see_one_wrong_row():
    """The measure of the GPU tests: one row off by 1 % in 4 000 is 1.6e-4 of the whole matrix and 1e-2 of its row."""
    want = torch.randn(4000, 64, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    got = want.clone()
    got[1234] *= 1.01
    assert float((got - want).norm() / want.norm()) < 2e-4
    err, row = R.worst_row(got, want)
    assert row == 1234 and abs(err - 0.01) < 1e-9
    z = torch.zeros(3, 8, dtype=torch.float64)
    assert R.worst_row(z, z)[0] == 0.0
    bad = z.clone(); bad[2, 1] = 1e-30
    assert R.worst_row(bad, z) == (float("inf"), 2)
