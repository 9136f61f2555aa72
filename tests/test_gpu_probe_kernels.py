"""The probe-head kernels (lstm.hip, probe.hip) per row, column and clip, off the shapes of test_gpu_probes.py.

test_gpu_probes.py runs the LSTM at one clip per workgroup only (B <= 6), dense_f32 through its wrapper only (contiguous, aligned, ld == K)
under one norm over the whole matrix, layer_mix in one pass, seq_interp_linear at 96 channels, mha_f32's plain kernel up to 300 keys.  Here:

  * the LSTM at 2 and 4 clips per workgroup -- forced in child processes (lstm.hip reads AVEX_AMD_LSTM_LR once per process) and reached by
    the shipped rule in process -- with clip counts that are no multiple of the tile, both LDS requests above 64 KB, NaN containment,
    saturated gates, every thread layout's boundary, the refusals;
  * dense_f32 through the C entry point with leading dimensions larger than the matrices, misaligned bases, the partial K tile of the
    vector path; NaN and Inf through every activation (ReLU keeps a NaN, as torch.relu does);
  * layer_mix past one pass of its grid, 1 and 16 taps, weights that need the max subtraction; seq_interp_linear at 257 / 768 channels and
    Tin = 1; mha_f32's plain kernel at 2048 keys, and a clip whose keys are all masked on both attention kernels.

Bars: an fp32 kernel may differ from fp64 by FACTOR (4) x what a NumPy fp32 restatement of the same arithmetic differs by on the same inputs
(_probe_ref.py; the bar never sees device output), per clip (LSTM), per row and per column (dense), per (token, head) segment (attention).
Every test prints ``PROBE <group> <case> device <worst> bar <bar>``.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attention_ref as A
import _probe_ref as R
from _util import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _host(t):
    return t.detach().float().cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _n_cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _report(group, case, worst_d, bar):
    print(f"PROBE {group} {case} device {worst_d:.3e} bar {bar:.3e}")


# =================================================================================================================================
# LSTM
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def _lstm_case(B, T, H, saturated=False):
    """(inputs, fp64 reference [B, T, 2H], bar): computed once per shape, never changed."""
    inp = R.lstm_saturated_inputs(B, T, H) if saturated else R.lstm_inputs(B, T, H)
    r64, r32 = R.lstm_refs(*inp)
    bar, n_floor, n = R.lstm_bar(r64, r32)
    A.assert_floor_cap(n_floor, n)
    return inp, r64, bar


def _lstm_check(out, r64, bar, group, case):
    """Every clip of each direction of ``out [B, T, 2H]`` against fp64."""
    H = r64.shape[-1] // 2
    worst_d = 0.0
    for d, sl in enumerate((slice(0, H), slice(H, 2 * H))):
        err, _ = R.clip_errors(out[..., sl], r64[..., sl])
        worst_d = max(worst_d, R.worst(err))
        assert R.worst(err) <= bar, (f"{group} {case} direction {d}: clip {int(np.argmax(np.where(np.isnan(err), np.inf, err)))} of {err.size} is off by "
                                     f"{R.worst(err):.3e} against {R.FACTOR:g} x the fp32 restatement's worst clip = {bar:.3e}")
    _report(group, case, worst_d, bar)
    return worst_d


def _lstm_pair(inp):
    from avex_amd import kernels as K
    xg, w, xgr, wr = [_dev(a) for a in inp]
    out = torch.full((xg.shape[0], xg.shape[1], 2 * w.shape[0]), NAN, dtype=torch.float32, device="cuda")
    K.lstm_layer_pair(xg, w, xgr, wr, out)
    return _host(out)


def _lstm_singles(inp):
    from avex_amd import kernels as K
    xg, w, xgr, wr = [_dev(a) for a in inp]
    out = torch.full((xg.shape[0], xg.shape[1], 2 * w.shape[0]), NAN, dtype=torch.float32, device="cuda")
    K.lstm_layer(xg, w, out, col=0, reverse=False)
    K.lstm_layer(xgr, wr, out, col=w.shape[0], reverse=True)
    return _host(out)


def _lstm_chunked(inp, chunk, pair):
    """The same clips in launches of at most ``chunk`` clips."""
    B = inp[0].shape[0]
    parts = []
    for b0 in range(0, B, chunk):
        sub = tuple(a if a.ndim == 2 else a[b0:b0 + chunk] for a in inp)
        parts.append(_lstm_pair(sub) if pair else _lstm_singles(sub))
    return np.concatenate(parts, axis=0)


# ---- forced tiling, one child process per value --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced_lr(built_lib, tmp_path_factory):
    """tests/tools/lstm_forced_lr.py three times, one after the other, each a fresh process under its own timeout (the switch is read once
    per process; a process that has opened the GPU never replaces its program).  The first child that fails ends the fixture."""
    tmp = tmp_path_factory.mktemp("lstm_forced_lr")
    res = {}
    for lr in (1, 2, 4):
        path = str(tmp / f"lr{lr}.npz")
        env = dict(os.environ, AVEX_AMD_LSTM_LR=str(lr))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "lstm_forced_lr.py"), path], capture_output=True, text=True, timeout=240,
                           env=env)
        assert r.returncode == 0, f"LR={lr}: exit {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]
        with np.load(path) as z:
            res[lr] = {k: z[k] for k in z.files}
        assert int(res[lr]["lr"]) == lr
    return res


@pytest.mark.parametrize("lr", [1, 2, 4])
def test_lstm_forced_tiling_against_fp64(forced_lr, lr):
    """1, 2 and 4 clips per workgroup at clip counts with remainders 1, 2, 3 against four, in all four thread layouts (H = 256 and 37 / 1:
    four threads per unit, 300: three, 512: two, 1024: one), with the two LDS requests above 64 KB (LR = 4 at H = 256: 69 632 B, at
    H = 1024: 81 920 B).  Per clip against fp64; the pair launch bit-equal to the two single launches; the four clips behind the last one
    given to the kernel still NaN."""
    G = R.LSTM_GUARD_CLIPS
    for B, H in R.LSTM_FORCED_CASES:
        _, r64, bar = _lstm_case(B, R.LSTM_T, H)
        single, pair = forced_lr[lr][f"single_{B}_{H}"], forced_lr[lr][f"pair_{B}_{H}"]
        assert single.shape == (B + G, R.LSTM_T, 2 * H) and pair.shape == single.shape
        for name, buf in (("single", single), ("pair", pair)):
            assert np.isnan(buf[B:]).all(), f"LR={lr} B={B} H={H} {name}: the kernel wrote behind clip B - 1"
        _lstm_check(single[:B], r64, bar, "lstm_forced", f"LR={lr} B={B} H={H}")
        assert _same_bits(pair[:B], single[:B]), f"LR={lr} B={B} H={H}: the pair launch differs from the two single launches"


def test_lstm_forced_tiling_bit_equal_across_lr(forced_lr):
    """A clip's arithmetic does not depend on the tile: the same FMA chain over k, the same order of the partial sums."""
    for B, H in R.LSTM_FORCED_CASES:
        for lr in (2, 4):
            a, b = forced_lr[lr][f"single_{B}_{H}"][:B], forced_lr[1][f"single_{B}_{H}"][:B]
            assert _same_bits(a, b), f"B={B} H={H}: LR={lr} differs from LR=1 by up to {np.abs(a.astype(np.float64) - b).max():.3e}"


# ---- the shipped selection rule, in process ---------------------------------------------------------------------------------------------
def _rule_case(name):
    n = _n_cu()
    dirs, B, lr = {"pair_n-1": (2, n - 1, 2), "pair_n+1": (2, n + 1, 4), "single_n+1": (1, n + 1, 2), "single_2n+1": (1, 2 * n + 1, 4)}[name]
    assert os.environ.get("AVEX_AMD_LSTM_LR", "") not in ("1", "2", "4"), "AVEX_AMD_LSTM_LR overrides the rule under test"
    assert R.lstm_clips_per_workgroup(B, dirs, n) == lr, (name, n)
    assert R.lstm_clips_per_workgroup(n // 2, dirs, n) == 1
    return dirs, B, lr, n


@pytest.mark.parametrize("name", ["pair_n-1", "pair_n+1", "single_n+1", "single_2n+1"])
def test_lstm_shipped_rule_reaches_the_tiles(built_lib, name):
    """Clip counts around the CU count reach 2 and 4 clips per workgroup by lstm_launch's own rule (restated in _probe_ref, asserted before
    anything is launched).  Bit-equal to the same clips in launches of at most n_cu / 2 clips (one clip per workgroup by the same rule), and
    every clip -- the first, the last, the last of a full workgroup among them -- against fp64."""
    dirs, B, lr, n = _rule_case(name)
    T, H = R.LSTM_RULE_TH
    inp, r64, bar = _lstm_case(B, T, H)
    pair = dirs == 2
    out = _lstm_pair(inp) if pair else _lstm_singles(inp)
    small = _lstm_chunked(inp, n // 2, pair)
    assert _same_bits(out, small), f"{name}: LR={lr} differs from LR=1 by up to {np.nanmax(np.abs(out.astype(np.float64) - small)):.3e}"
    _lstm_check(out, r64, bar, "lstm_rule", f"{name} B={B} LR={lr}")
    for b in (0, B - 1, (B // lr) * lr - 1):
        assert np.isfinite(out[b]).all()
        _lstm_check(out[b:b + 1], r64[b:b + 1], bar, "lstm_rule", f"{name} clip {b}")


def test_lstm_nan_stays_in_its_clip_and_direction(built_lib):
    """Four clips per workgroup share one LDS copy of h: a NaN step of one clip (in the middle of a workgroup, and the last clip, whose
    workgroup is padded with repeats of it) makes that clip NaN from that step on -- the later steps forward, the earlier ones in reverse --
    and leaves every other clip bit-equal to the clean run."""
    dirs, B, lr, n = _rule_case("pair_n+1")
    T, H = R.LSTM_RULE_TH
    inp, _, _ = _lstm_case(B, T, H)
    clean = _lstm_pair(inp)
    t0, hit = 1, (5, B - 1)
    xg, w, xgr, wr = [a.copy() for a in inp]
    for b in hit:
        xg[b, t0] = np.nan
        xgr[b, t0] = np.nan
    out = _lstm_pair((xg, w, xgr, wr))
    others = np.setdiff1d(np.arange(B), hit)
    assert _same_bits(out[others], clean[others]), "a NaN left its clip"
    for b in hit:
        assert np.isnan(out[b, t0:, :H]).all() and _same_bits(out[b, :t0, :H], clean[b, :t0, :H]), f"forward, clip {b}"
        assert np.isnan(out[b, :t0 + 1, H:]).all() and _same_bits(out[b, t0 + 1:, H:], clean[b, t0 + 1:, H:]), f"reverse, clip {b}"


def test_lstm_saturated_gates(built_lib):
    """xg stretched to +-60: exp(60) in the sigmoids, tanh at its ends.  Finite, and within the bar."""
    dirs, B, lr, n = _rule_case("pair_n+1")
    T, H = R.LSTM_RULE_TH
    inp, r64, bar = _lstm_case(B, T, H, True)
    assert max(np.abs(inp[0]).max(), np.abs(inp[2]).max()) == pytest.approx(60.0) and (np.abs(inp[0]) > 20).mean() > 0.1
    out = _lstm_pair(inp)
    assert np.isfinite(out).all()
    _lstm_check(out, r64, bar, "lstm_saturated", f"B={B}")


@pytest.mark.parametrize("H", R.LSTM_BOUNDARY_H)
def test_lstm_layout_boundaries(built_lib, H):
    """Both sides of every thread-layout boundary (four / three / two / one thread per hidden unit) and the widest layer."""
    B, T = R.LSTM_BOUNDARY_BT
    inp, r64, bar = _lstm_case(B, T, H)
    out = _lstm_singles(inp)
    _lstm_check(out, r64, bar, "lstm_boundary", f"H={H}")
    assert _same_bits(_lstm_pair(inp), out)


def test_lstm_refusals(built_lib):
    """H > 1024, T = 0 and ldo < H are refused before anything is launched (NaN canary); B = 0 is fine and writes nothing."""
    from avex_amd._capi import lib
    xg = torch.zeros((2 * 3 * 4 * 1025,), dtype=torch.float32, device="cuda")
    w = torch.zeros((1025 * 4 * 1025,), dtype=torch.float32, device="cuda")
    out = torch.full((2 * 3 * 2 * 1025,), NAN, dtype=torch.float32, device="cuda")
    p = lambda t: t.data_ptr()
    L = lib()
    assert L.avexhip_lstm_layer(p(xg), p(w), 2, 3, 1025, 0, p(out), 1025, _stream()) != 0
    assert L.avexhip_lstm_layer(p(xg), p(w), 2, 0, 64, 0, p(out), 64, _stream()) != 0
    assert L.avexhip_lstm_layer(p(xg), p(w), 2, 3, 64, 0, p(out), 63, _stream()) != 0
    assert L.avexhip_lstm_layer_pair(p(xg), p(w), p(xg), p(w), 2, 3, 1025, p(out), p(out) + 4 * 1025, 2050, _stream()) != 0
    assert L.avexhip_lstm_layer_pair(p(xg), p(w), p(xg), p(w), 2, 0, 64, p(out), p(out) + 4 * 64, 128, _stream()) != 0
    assert L.avexhip_lstm_layer_pair(p(xg), p(w), p(xg), p(w), 2, 3, 64, p(out), p(out) + 4 * 64, 63, _stream()) != 0
    assert L.avexhip_lstm_layer(p(xg), p(w), 0, 3, 64, 0, p(out), 64, _stream()) == 0
    assert L.avexhip_lstm_layer_pair(p(xg), p(w), p(xg), p(w), 0, 3, 64, p(out), p(out) + 4 * 64, 128, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# =================================================================================================================================
# dense_f32 through the C entry point
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def _dense_case(M, N, K, act):
    x, w, b, r = R.dense_inputs(M, N, K)
    r64, row_bar, col_bar, n_floor, n = R.dense_bars(x, w, b, act, r)
    A.assert_floor_cap(n_floor, n)
    return (x, w, b, r), r64, row_bar, col_bar


def _padded(a, ld, off):
    """``a [R, C]`` as rows of a NaN-filled flat buffer: row stride ``ld``, first element ``off`` floats behind the (512-byte aligned)
    base.  Returns (buffer, address of a[0, 0])."""
    rows, cols = a.shape
    buf = torch.full((off + rows * ld,), NAN, dtype=torch.float32, device="cuda")
    buf[off:].view(rows, ld)[:, :cols] = _dev(a)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * off


def _dense_raw(x, w, b, r, act, ldx, ldw, off=0, ldo_pad=5, ldr_pad=2, extra_rows=3):
    """avexhip_dense_f32 on views into larger, NaN-filled buffers; checks that nothing outside out[:M, :N] was written."""
    from avex_amd._capi import lib, check
    from avex_amd.kernels import PROBE_ACT
    M, K = x.shape
    N = w.shape[0]
    ldo, ldr = N + ldo_pad, N + ldr_pad
    xb, xp = _padded(x, ldx, off)
    wb, wp = _padded(w, ldw, off)
    rb, rp = _padded(r, ldr, 0)
    bias = _dev(b)
    out = torch.full((M + extra_rows, ldo), NAN, dtype=torch.float32, device="cuda")
    check(lib().avexhip_dense_f32(xp, ldx, wp, ldw, bias.data_ptr(), rp, ldr, M, N, K, PROBE_ACT[act], out.data_ptr(), ldo, _stream()), "dense_f32")
    got = _host(out)
    assert np.isnan(got[:M, N:]).all(), "dense_f32 wrote into the padding columns of out"
    assert np.isnan(got[M:]).all(), "dense_f32 wrote behind row M - 1"
    return got[:M, :N]


def _dense_layouts(K):
    """(name, ldx, ldw, base offset in floats, vector loads expected)."""
    return (("ldx+3_ldw+1", K + 3, K + 1, 0, False),                  # leading dimensions that are no multiple of 4: scalar loads
            ("ldx+4_ldw+1", K + 4, K + 1, 0, False),
            ("ldx+4_ldw+8", K + 4, K + 8, 0, K % 4 == 0),             # the vector path with ld > K (and its partial K tile at K = 4, 20, 36)
            ("ldx+4_ldw+4_base+1", K + 4, K + 4, 1, False))           # 4-byte aligned, not 16-byte aligned: scalar loads although K % 4 == 0


def _dense_check(got, r64, row_bar, col_bar, case):
    er, _ = R.row_errors(got, r64)
    ec, _ = R.col_errors(got, r64)
    _report("dense_row", case, R.worst(er), row_bar)
    _report("dense_col", case, R.worst(ec), col_bar)
    assert R.worst(er) <= row_bar, f"{case}: row {int(np.argmax(np.where(np.isnan(er), np.inf, er)))} off by {R.worst(er):.3e}, bar {row_bar:.3e}"
    assert R.worst(ec) <= col_bar, f"{case}: column {int(np.argmax(np.where(np.isnan(ec), np.inf, ec)))} off by {R.worst(ec):.3e}, bar {col_bar:.3e}"


@pytest.mark.parametrize("K", R.DENSE_K)
@pytest.mark.parametrize("M", R.DENSE_MN)
def test_dense_leading_dimensions(built_lib, M, K):
    """One row / column short of, at, and one past the 128 tile, K below, at and past the 16-deep K tile (4, 20, 36: the vector path's
    partial tile; 17: scalar), operands with leading dimensions past K and N whose padding is NaN (a load that strays into it poisons its
    row), every activation with bias and residual.  Per row and per column against fp64."""
    for N in R.DENSE_MN:
        for act in R.ACTS:
            (x, w, b, r), r64, row_bar, col_bar = _dense_case(M, N, K, act)
            for name, ldx, ldw, off, vec in _dense_layouts(K):
                assert vec == (K % 4 == 0 and ldx % 4 == 0 and ldw % 4 == 0 and off % 4 == 0)
                got = _dense_raw(x, w, b, r, act, ldx, ldw, off)
                _dense_check(got, r64, row_bar, col_bar, f"M={M} N={N} K={K} {act} {name}")


@pytest.mark.parametrize("act", R.ACTS)
def test_dense_two_tiles_long_chain(built_lib, act):
    M, N, K = R.DENSE_LONG
    (x, w, b, r), r64, row_bar, col_bar = _dense_case(M, N, K, act)
    for name, ldx, ldw, off, vec in _dense_layouts(K):
        _dense_check(_dense_raw(x, w, b, r, act, ldx, ldw, off), r64, row_bar, col_bar, f"M={M} N={N} K={K} {act} {name}")


# ---- NaN and Inf -------------------------------------------------------------------------------------------------------------------------
EDGES = (31, 32, 127, 128)      # both sides of a 32-row MFMA block edge and of the 128 tile edge


@pytest.mark.parametrize("act", R.ACTS)
def test_dense_nan_stays_in_its_row_and_column(built_lib, act):
    """A NaN in x[m0, k0] makes exactly row m0 NaN -- under ReLU too, as torch.relu and the oracle's np.maximum do -- and a NaN in w[n0, :]
    exactly column n0; everything else bit-equal to the clean run."""
    from avex_amd import kernels as K
    M, N, Kd = 161, 160, 20
    x, w, b, r = R.dense_inputs(M, N, Kd)
    run = lambda x_, w_: _host(K.dense_f32(_dev(x_), _dev(w_), _dev(b), act=act, resid=_dev(r)))
    clean = run(x, w)
    assert np.isfinite(clean).all()
    for i, e in enumerate(EDGES):
        x2 = x.copy()
        x2[e, (3 * i) % Kd] = np.nan
        got = run(x2, w)
        keep = np.arange(M) != e
        assert np.isnan(got[e]).all(), f"{act}: NaN in x[{e}] did not reach all of row {e} ({int(np.isnan(got[e]).sum())} of {N})"
        assert _same_bits(got[keep], clean[keep]), f"{act}: NaN in x[{e}] changed another row"
        w2 = w.copy()
        w2[e, (5 * i + 1) % Kd] = np.nan
        got = run(x, w2)
        keep = np.arange(N) != e
        assert np.isnan(got[:, e]).all(), f"{act}: NaN in w[{e}] did not reach all of column {e}"
        assert _same_bits(got[:, keep], clean[:, keep]), f"{act}: NaN in w[{e}] changed another column"
    without_resid = _host(K.dense_f32(_dev(x2), _dev(w), _dev(b), act=act))      # (no residual to carry the NaN)
    assert np.isnan(without_resid[EDGES[-1]]).all() and np.isfinite(np.delete(without_resid, EDGES[-1], axis=0)).all()


def test_dense_inf_through_relu_and_tanh(built_lib):
    """+Inf under ReLU stays +Inf and is 1 under tanh; -Inf is 0 under ReLU (either zero) and -1 under tanh."""
    from avex_amd import kernels as K
    M, N, Kd = 40, 33, 20
    x, w, b, _ = R.dense_inputs(M, N, Kd)
    w = w.copy()
    w[:, 7] = np.abs(w[:, 7]) + np.float32(0.1)      # a positive column: the sign of x[m, 7] = +-Inf is the sign of the whole row
    x = x.copy()
    x[31, 7], x[32, 7] = np.inf, -np.inf
    relu = _host(K.dense_f32(_dev(x), _dev(w), _dev(b), act="relu"))
    tanh = _host(K.dense_f32(_dev(x), _dev(w), _dev(b), act="tanh"))
    assert (relu[31] == np.inf).all() and (relu[32] == 0.0).all()
    assert (tanh[31] == 1.0).all() and (tanh[32] == -1.0).all()
    keep = np.setdiff1d(np.arange(M), (31, 32))
    assert np.isfinite(relu[keep]).all() and np.isfinite(tanh[keep]).all()


@pytest.mark.parametrize("act", ["relu", "gelu", "tanh"])
def test_mlp_probe_keeps_a_nan_clip(built_lib, act):
    """MLPProbe has no residual: the activation alone decides whether a NaN embedding reaches the logits."""
    from avex_amd import probes as P
    gen = torch.Generator().manual_seed(11)
    pr = P.MLPProbe(None, [], 7, feature_mode=True, input_dim=48, hidden_dims=[40, 24], dropout_rate=0.1, activation=act)
    pr.load_state_dict({k: (torch.randn(v.shape, generator=gen) * (0.3 if v.dim() == 1 else v.shape[-1] ** -0.5)).cuda() for k, v in pr.state_dict().items()})
    x = torch.randn(6, 48, generator=gen)
    clean = _host(pr(x.cuda()))
    x[4, 17] = NAN
    got = _host(pr(x.cuda()))
    keep = np.arange(6) != 4
    assert np.isfinite(clean).all() and np.isnan(got[4]).all(), f"{act}: logits of the NaN clip: {got[4]}"
    assert _same_bits(got[keep], clean[keep])


# =================================================================================================================================
# layer_mix
# =================================================================================================================================
def _mix_loop(taps, w=None):
    ref = torch.zeros_like(taps[0])
    for i, t in enumerate(taps):
        ref = ref + (1.0 if w is None else w[i]) * t
    return ref


def test_layer_mix_second_pass_of_the_grid(built_lib):
    """8192 workgroups of 256 threads: elements from 2 097 152 on are a thread's second element."""
    from avex_amd import kernels as K
    n = 8192 * 256 + 300
    g = torch.Generator().manual_seed(1)
    taps = [torch.randn(n, generator=g).cuda() for _ in range(2)]
    out, ref = K.layer_mix(taps), _mix_loop(taps)
    assert torch.equal(out[-300:], ref[-300:]), "the elements of the second pass"
    assert torch.equal(out[:300], ref[:300]), "the first elements"
    assert torch.equal(out, ref)


def test_layer_mix_tap_counts_and_weight_range(built_lib):
    from avex_amd import kernels as K
    g = torch.Generator().manual_seed(2)
    taps = [torch.randn(5, 333, generator=g).cuda() for _ in range(16)]
    # one tap: softmax of one weight is exactly 1
    assert torch.equal(K.layer_mix(taps[:1], torch.tensor([0.37]).cuda()), taps[0])
    assert torch.equal(K.layer_mix(taps[:1]), taps[0])
    # sixteen taps, the most there are
    assert torch.equal(K.layer_mix(taps), _mix_loop(taps))
    lw = torch.randn(16, generator=g)
    w64 = torch.softmax(lw.double(), 0)
    ref = sum(w64[i] * taps[i].double().cpu() for i in range(16))
    assert rel_l2(_host(K.layer_mix(taps, lw.cuda())), ref.numpy()) < 3e-7
    # weights that overflow exp() without the max subtraction: e^0, e^-1, 0 before normalising
    lw = torch.tensor([1000.0, 999.0, -1000.0])
    w64 = torch.softmax(lw.double(), 0)
    assert w64[2] == 0.0
    ref = sum(w64[i] * taps[i].double().cpu() for i in range(3))
    out = _host(K.layer_mix(taps[:3], lw.cuda()))
    assert np.isfinite(out).all() and rel_l2(out, ref.numpy()) < 3e-7


def test_layer_mix_nan_and_refusal(built_lib):
    from avex_amd import kernels as K
    from avex_amd._capi import lib
    g = torch.Generator().manual_seed(3)
    taps = [torch.randn(2000, generator=g).cuda() for _ in range(3)]
    lw = torch.randn(3, generator=g).cuda()
    clean = _host(K.layer_mix(taps, lw))
    taps[1][1234] = NAN
    got = _host(K.layer_mix(taps, lw))
    keep = np.arange(2000) != 1234
    assert np.isnan(got[1234]) and _same_bits(got[keep], clean[keep])
    many = [taps[0]] * 17
    with pytest.raises(ValueError):
        K.layer_mix(many)
    out = torch.full((2000,), NAN, dtype=torch.float32, device="cuda")
    arr = (C.c_void_p * 17)(*[t.data_ptr() for t in many])
    assert lib().avexhip_layer_mix(arr, 17, None, 2000, out.data_ptr(), _stream()) != 0
    assert lib().avexhip_layer_mix(arr, 0, None, 2000, out.data_ptr(), _stream()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# =================================================================================================================================
# seq_interp_linear
# =================================================================================================================================
def _interp_taps(Tin, Tout):
    """(i0, i1) per output row by the kernel's formula in fp32; asserted not to depend on whether the compiler contracts
    ``scale * (t + 0.5) - 0.5`` into one FMA."""
    t = np.arange(Tout, dtype=np.float32)
    scale = np.float32(Tin) / np.float32(Tout)
    src = (scale * (t + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    fma = (np.float64(scale) * (t.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    src, fma = np.maximum(src, np.float32(0.0)), np.maximum(fma, np.float32(0.0))
    i0 = src.astype(np.int64)
    assert np.array_equal(i0, fma.astype(np.int64)), "pick sizes whose source positions are not within an ulp of an integer"
    return i0, i0 + (i0 < Tin - 1)


@pytest.mark.parametrize("Tin,Tout", R.INTERP_T)
@pytest.mark.parametrize("Cc", R.INTERP_C)
def test_seq_interp_wide_rows(built_lib, Cc, Tin, Tout):
    """More channels than the 256 threads of a workgroup (257: one thread makes a second pass; 768: the real tap width), a single input
    step, a single output step, and the encoder's 1496 -> 496: against torch's interpolate at the bars of test_gpu_probes.py, whole and per
    output row."""
    from avex_amd import kernels as K
    x = torch.from_numpy(R.interp_input(Tin, Cc))
    ref = torch.nn.functional.interpolate(x.transpose(1, 2), size=Tout, mode="linear", align_corners=False).transpose(1, 2)
    got = K.seq_interp_linear(x.cuda(), Tout).cpu()
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 2e-5 and rel_l2(got.numpy(), ref.numpy()) < 2e-6
    err, n_floor = R.row_errors(got.numpy().reshape(2 * Tout, Cc), ref.numpy().reshape(2 * Tout, Cc))
    A.assert_floor_cap(n_floor, err.size)
    _report("seq_interp_row", f"C={Cc} {Tin}->{Tout}", R.worst(err), 2e-6)
    assert R.worst(err) < 2e-6, f"row {int(np.argmax(err))}"


@pytest.mark.parametrize("Cc,Tin,Tout", [(257, 41, 24), (768, 1496, 496), (257, 24, 41)])
def test_seq_interp_nan_reaches_its_rows_only(built_lib, Cc, Tin, Tout):
    """A NaN in one input element reaches the output rows that read its step as i0 or i1 (whatever the weight: 0 x NaN is NaN), in its
    channel only.  Sizes whose source positions are never integers in exact arithmetic (41 / 24 and 187 / 62 times odd halves)."""
    from avex_amd import kernels as K
    x = R.interp_input(Tin, Cc).copy()
    clean = _host(K.seq_interp_linear(_dev(x), Tout))
    i0, i1 = _interp_taps(Tin, Tout)
    t0, c0 = int(i1[Tout // 2]), Cc - 1            # a step that some output row reads (downsampling skips steps); a channel of the last pass
    x[1, t0, c0] = np.nan
    got = _host(K.seq_interp_linear(_dev(x), Tout))
    rows = (i0 == t0) | (i1 == t0)
    assert rows.any() and not rows.all()
    expect = np.zeros(got.shape, bool)
    expect[1, rows, c0] = True
    assert np.array_equal(np.isnan(got), expect), f"NaN rows {np.flatnonzero(np.isnan(got[1, :, c0]))}, expected {np.flatnonzero(rows)}"
    assert _same_bits(got[~expect], clean[~expect])


# =================================================================================================================================
# mha_f32
# =================================================================================================================================
def test_mha_plain_kernel_at_its_longest(built_lib):
    """Head width 4 takes the kernel without the matrix core; 2048 keys is its admitted maximum: 16 x 128 + 16 x 2048 floats = 139 264 B
    of LDS.  Per (token, head) segment with the bars of test_segment_parity_mha_f32.  One key more is refused."""
    from avex_amd import kernels as K
    from avex_amd._capi import AvexHipError
    B, T, H, D = R.MHA_LONG
    qkv = A.random_case(B, T, H, D, "f32")
    for pad in (None, A.pad_mask(B, T)):
        out = _host(K.mha_f32(_dev(qkv).reshape(B, T, 3 * H * D), H, None if pad is None else _dev(pad.astype(np.uint8), torch.uint8)))
        out = out.reshape(B * T, H * D)
        ref = A.plain_attention_ref(qkv, B, T, H, D, key_pad=pad)
        emu = A.mha_f32_restatement(qkv, B, T, H, D, key_pad=pad)
        err_e, n_floor = A.segment_errors(emu, ref, H, D)
        A.assert_floor_cap(n_floor, err_e.size)
        err_d, _ = A.segment_errors(out, ref, H, D)
        worst_e, _ = A.worst_segment(err_e)
        worst_d, (r, h) = A.worst_segment(err_d)
        _report("mha_f32", f"T={T} D={D} mask={int(pad is not None)}", worst_d, R.FACTOR * worst_e)
        assert worst_d <= R.FACTOR * worst_e, f"token {r} head {h}: {worst_d:.3e} against {R.FACTOR:g} x {worst_e:.3e}"
    with pytest.raises(AvexHipError, match="2048"):
        K.mha_f32(torch.zeros((1, 2049, 24), dtype=torch.float32, device="cuda"), 2)


@pytest.mark.parametrize("T", [40, 130])
@pytest.mark.parametrize("D", [4, 32])
def test_mha_fully_masked_clip(built_lib, D, T):
    """A clip with every key masked is NaN on both kernels (head width 4: the plain one, 32: the matrix-core one), as it is from
    nn.MultiheadAttention; its neighbours are bit-equal to a run without the mask."""
    from avex_amd import kernels as K
    B, H = 3, 2
    qkv = _dev(A.random_case(B, T, H, D, "f32")).reshape(B, T, 3 * H * D)
    pad = torch.zeros((B, T), dtype=torch.uint8, device="cuda")
    pad[1] = 1
    got, free = _host(K.mha_f32(qkv, H, pad)), _host(K.mha_f32(qkv, H, None))
    assert np.isnan(got[1]).all(), f"{int(np.isfinite(got[1]).sum())} finite values in the masked clip"
    assert np.isfinite(free).all() and _same_bits(got[[0, 2]], free[[0, 2]])
