"""tests/_rows_ref.py (the restatements tests/test_gpu_rows.py compares the row kernels with) against torch on the CPU, on tiny shapes:
LayerNorm and its token mean, the swish gate, the maximum with NaN, the order-exact mean, the Toeplitz gather, the ulp helpers.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rows_ref as R
from _util import round_half
from avex_amd import synth


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize("C", [4, 12, 264])
def test_layer_norm_matches_torch_fp64(C):
    x = synth.normal(f"rr_ln{C}", (5, C), 2.0).astype(np.float64) + 0.5
    x[1] = 3.25                                           # constant row: exactly the bias
    x[2] = 0.0
    w = 1.0 + synth.normal("rr_w", (C,), 0.1).astype(np.float64)
    b = synth.normal("rr_b", (C,), 0.1).astype(np.float64)
    want = F.layer_norm(_t(x), (C,), _t(w), _t(b), 1e-5).numpy()
    got = R.layer_norm(x, w, b, 1e-5)
    assert np.abs(got - want).max() < 1e-13
    assert np.array_equal(got[1], b) and np.array_equal(got[2], b)
    rstd = R.row_rstd(x, 1e-5)
    assert np.allclose((x - x.mean(-1, keepdims=True)) * rstd * w + b, want, rtol=0, atol=1e-13)


def test_layer_norm_pool_is_the_token_mean_of_layer_norm():
    B, T, C = 2, 7, 16
    x = synth.normal("rr_lnp", (B, T, C), 1.5).astype(np.float64)
    w = 1.0 + synth.normal("rr_w", (C,), 0.1).astype(np.float64)
    b = synth.normal("rr_b", (C,), 0.1).astype(np.float64)
    want = F.layer_norm(_t(x), (C,), _t(w), _t(b), 1e-6).mean(dim=1).numpy()
    assert np.abs(R.layer_norm_pool(x, w, b, 1e-6) - want).max() < 1e-13


def test_glu_swish_matches_silu_and_does_not_overflow():
    g = np.array([0.0, 2.0 ** -14, -2.0 ** -14, -20.0, 100.0, -100.0, -65504.0, 0.7, -3.0, 30.0, -700.0, 700.0], np.float64)
    a = synth.normal("rr_glu", (3, g.size), 2.0).astype(np.float64)
    y = np.concatenate([a, np.broadcast_to(g, a.shape)], axis=1)
    with np.errstate(over="raise", divide="raise"):       # no overflow inside the restatement, at any gate value
        got = R.glu_swish(y)
    want = (_t(a) * F.silu(_t(np.broadcast_to(g, a.shape).copy()))).numpy()
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    assert got.shape == (3, g.size)
    # a = inf against a gate whose swish is exactly zero: NaN, as in torch
    y2 = np.array([[np.inf, np.inf, 1.0, 0.0, -1e300, 3.0]], np.float64)
    got2 = R.glu_swish(y2)
    want2 = (_t(y2[:, :3]) * F.silu(_t(y2[:, 3:]))).numpy()
    assert np.array_equal(np.isnan(got2), np.isnan(want2)) and np.isnan(got2[0, 0])


def test_max_pool_keeps_nan_like_torch_max():
    x = synth.normal("rr_max", (2, 5, 6), 1.0)
    x[0, 3, 2] = np.nan
    x[1, :, 4] = -np.inf
    x[1, 0, 5] = np.nan
    want = _t(x).max(dim=1)[0].numpy()
    got = R.max_pool(x)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[0, 2]) and np.isnan(got[1, 5]) and got[1, 4] == -np.inf and np.isnan(got).sum() == 2


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 9])
def test_mean_pool_f32_is_the_stated_order(T):
    """Against a scalar loop that spells the order out, and within fp32 rounding of the fp64 mean."""
    B, C = 2, 3
    x = synth.normal(f"rr_mp{T}", (B, T, C), 1.0)
    got = R.mean_pool_f32(x)
    assert got.dtype == np.float32
    for b in range(B):
        for c in range(C):
            p = [np.float32(0.0)] * 4
            for t in range(T):
                p[t % 4] = np.float32(p[t % 4] + x[b, t, c])
            want = np.float32(np.float32(np.float32(p[0] + p[1]) + np.float32(p[2] + p[3])) / np.float32(T))
            assert got[b, c] == want
    assert np.abs(got - x.mean(axis=1, dtype=np.float64)).max() < 1e-6
    if T <= 4:      # one addend per phase: the fp32 sum tree of torch's own values
        xt = _t(x)
        tot = xt[:, 0]
        if T == 2:
            tot = xt[:, 0] + xt[:, 1]
        elif T == 3:
            tot = (xt[:, 0] + xt[:, 1]) + xt[:, 2]
        elif T == 4:
            tot = (xt[:, 0] + xt[:, 1]) + (xt[:, 2] + xt[:, 3])
        assert np.array_equal(got, (tot / T).numpy())


def test_toeplitz_is_the_clamped_gather():
    nb, H, maxd, T = 6, 3, 4, 9
    table = synth.normal("rr_tab", (nb, H), 1.0)
    lut = (np.arange(2 * maxd + 1) * 5 % nb).astype(np.int32)
    got = R.toeplitz(table, lut, maxd, T)
    assert got.shape == (H, 2 * T - 1) and got.dtype == table.dtype
    for h in range(H):
        for r in range(2 * T - 1):
            d = min(max(r - (T - 1), -maxd), maxd)
            assert got[h, r] == table[lut[d + maxd], h]


def test_row_sums_and_lnr_fold():
    w = round_half(synth.normal("rr_rs", (3, 65), 0.1), "bf16")
    assert np.array_equal(R.row_sums(w), _t(w).double().sum(dim=1).numpy())
    g, be, bi = (synth.normal(n, (5,), 1.0) for n in ("rr_g", "rr_be", "rr_bi"))
    ga, bb = R.lnr_fold(g, be, bi, 1.7)
    a = float(np.float32(1.7))
    assert np.array_equal(ga, g.astype(np.float64) * a) and np.array_equal(bb, bi.astype(np.float64) + a * be.astype(np.float64))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_half_ulp_matches_torch_spacing(dtype):
    td = torch.float16 if dtype == "f16" else torch.bfloat16
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 1000.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 0.0, -3.0], dtype=torch.float32).to(td)
    nxt = torch.nextafter(v.abs(), torch.tensor(float("inf"), dtype=td))
    want = (nxt.double() - v.abs().double()).numpy()
    assert np.array_equal(R.half_ulp(v.double().numpy(), dtype), want)
    f = np.array([1.0, 3.0, 1e-3, 1e4, 0.0], np.float32)
    assert np.array_equal(R.f32_ulp(f), np.nextafter(np.abs(f), np.float32(np.inf)).astype(np.float64) - np.abs(f).astype(np.float64))
