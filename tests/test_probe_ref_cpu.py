"""The references and instruments of the probe-kernel tests (_probe_ref.py) checked without a GPU: the fp64 references against torch in
double, the per-row / per-column / per-clip instruments against corruptions that the whole-array norms of test_gpu_probes.py cannot see, the
restated tiling rule of lstm.hip, and that no reference of test_gpu_probe_kernels.py has a segment under the norm floor."""
import numpy as np
import pytest
import torch

import _attention_ref as A
import _probe_ref as R
from _util import rel_l2

OLD_DENSE_BAR = 2e-6      # test_gpu_probes.py::test_dense_f32, one norm over the whole matrix
OLD_LSTM_BAR = 2e-5       # test_gpu_probes.py::test_lstm_layer_long_sequence, one norm over all clips


@pytest.mark.parametrize("B,T,D,H", [(3, 7, 5, 4), (2, 5, 3, 37)])
def test_lstm_ref_matches_torch_in_double(B, T, D, H):
    torch.manual_seed(B * 100 + H)
    lstm = torch.nn.LSTM(D, H, batch_first=True, bidirectional=True).double().eval()
    x = torch.randn(B, T, D, dtype=torch.float64)
    with torch.no_grad():
        ref, _ = lstm(x)
    for di, sfx in enumerate(("", "_reverse")):
        w_ih, w_hh = getattr(lstm, f"weight_ih_l0{sfx}").detach(), getattr(lstm, f"weight_hh_l0{sfx}").detach()
        b = (getattr(lstm, f"bias_ih_l0{sfx}") + getattr(lstm, f"bias_hh_l0{sfx}")).detach()
        xg = (x @ w_ih.T + b).numpy()
        got = R.lstm_ref(xg, w_hh.T.numpy(), reverse=bool(di), dtype=np.float64)
        assert np.abs(got - ref[..., di * H:(di + 1) * H].numpy()).max() < 1e-13
        # the fp32 restatement computes the same thing, to fp32
        low = R.lstm_ref(xg, w_hh.T.numpy(), reverse=bool(di), dtype=np.float32)
        assert low.dtype == np.float32 and rel_l2(low, got) < 1e-5


@pytest.mark.parametrize("act", R.ACTS)
def test_dense_ref_matches_torch_in_double(act):
    x, w, b, r = R.dense_inputs(9, 11, 13)
    x = x.copy()
    x[4, 6] = np.nan
    tx, tw, tb, tr = [torch.from_numpy(a).double() for a in (x, w, b, r)]
    y = torch.nn.functional.linear(tx, tw, tb)
    y = {None: y, "relu": torch.relu(y), "gelu": torch.nn.functional.gelu(y), "tanh": torch.tanh(y)}[act] + tr
    got = R.dense_ref(x, w, b, act, r, np.float64)
    assert np.isnan(got[4]).all() and torch.isnan(y[4]).all(), "a NaN stays a NaN under every activation, ReLU included"
    keep = np.arange(9) != 4
    assert np.isfinite(got[keep]).all() and np.abs(got[keep] - y.numpy()[keep]).max() < 1e-14
    low = R.dense_ref(x, w, b, act, r, np.float32)
    assert low.dtype == np.float32 and np.isnan(low[4]).all() and rel_l2(low[keep], got[keep]) < 1e-6
    assert np.array_equal(R.dense_ref(x[keep], w, None, None, None, np.float64), x[keep].astype(np.float64) @ w.astype(np.float64).T)


def test_relu_reference_semantics():
    """What the device ReLU has to do, on the two libraries the project compares with."""
    v = np.array([np.nan, -np.inf, np.inf, -1.0, 2.0], np.float32)
    for got in (R.activation(v, "relu"), torch.relu(torch.from_numpy(v)).numpy()):
        assert np.isnan(got[0]) and got[1] == 0.0 and got[2] == np.inf and got[3] == 0.0 and got[4] == 2.0
    assert R.activation(np.array([np.inf, -np.inf], np.float32), "tanh").tolist() == [1.0, -1.0]


def test_instruments_see_one_wrong_row_column_clip():
    """One row (column, clip) off by 1e-3 relative: the whole-array norm of the old tests stays under their bars when the array has enough
    rows (1e-3 / sqrt(rows)), the per-segment instrument does not.  The bar of each instrument is the one the GPU tests use: FACTOR x the
    fp32 restatement's worst segment."""
    M = 300_000
    x, w, b, r = R.dense_inputs(M, 4, 4)
    r64, row_bar, _, n_floor, n = R.dense_bars(x, w, b, "gelu", r)
    A.assert_floor_cap(n_floor, n)
    bad = r64.copy()
    m0 = int(np.argsort(np.linalg.norm(r64, axis=1))[M // 2])      # a row of median norm
    bad[m0] *= 1.0 + 1e-3
    err, _ = R.row_errors(bad, r64)
    assert rel_l2(bad, r64) < OLD_DENSE_BAR and R.worst(err) > row_bar and int(np.argmax(err)) == m0 and R.worst(err) == pytest.approx(1e-3, rel=1e-6)
    x, w, b, r = R.dense_inputs(4, M, 4)
    r64, _, col_bar, n_floor, n = R.dense_bars(x, w, b, "tanh", r)
    A.assert_floor_cap(n_floor, n)
    bad = r64.copy()
    n0 = int(np.argsort(np.linalg.norm(r64, axis=0))[M // 2])
    bad[:, n0] *= 1.0 + 1e-3
    err, _ = R.col_errors(bad, r64)
    assert rel_l2(bad, r64) < OLD_DENSE_BAR and R.worst(err) > col_bar and int(np.argmax(err)) == n0
    assert R.worst(R.row_errors(bad, r64)[0]) < 1e-3      # (spread over a row's 300 000 columns it is nothing: the instrument must match)
    B = 8192
    r64, r32 = R.lstm_refs(*R.lstm_inputs(B, 2, 2))
    bar, n_floor, n = R.lstm_bar(r64, r32)
    A.assert_floor_cap(n_floor, n)
    bad = r64.copy()
    b0 = int(np.argsort(np.linalg.norm(r64.reshape(B, -1), axis=1))[B // 2])
    bad[b0] *= 1.0 + 1e-3
    err, _ = R.clip_errors(bad, r64)
    assert rel_l2(bad, r64) < OLD_LSTM_BAR and R.worst(err) > bar and int(np.argmax(err)) == b0


def test_old_dense_shape_hides_a_wrong_row():
    """At the widest shape of test_dense_f32 (300 x 2304) a row off by 3e-5 -- a hundred times what fp32 costs it -- passes the old bar
    (3e-5 / sqrt(300) = 1.7e-6 < 2e-6) and fails the per-row one."""
    x, w, b, r = R.dense_inputs(300, 2304, 64)
    r64, row_bar, _, n_floor, n = R.dense_bars(x, w, b, None, r)
    A.assert_floor_cap(n_floor, n)
    assert row_bar < 3e-6
    bad = r64.copy()
    bad[177] *= 1.0 + 3e-5
    assert rel_l2(bad, r64) < OLD_DENSE_BAR and R.worst(R.row_errors(bad, r64)[0]) > row_bar


def test_instruments_floor_and_nan():
    ref = np.ones((200, 8))
    ref[3] *= 2.0 ** -8                                   # under 2^-6 x the median norm
    out = ref.copy()
    out[3] += 2.0 ** -8
    err, n_floor = R.row_errors(out, ref)
    assert n_floor == 1 and err[3] == pytest.approx(2.0 ** -8 / 2.0 ** -6) and (np.delete(err, 3) == 0).all()
    err, n_floor = R.col_errors(out.T, ref.T)
    assert n_floor == 1 and err[3] == pytest.approx(0.25)
    err, n_floor = R.clip_errors(out.reshape(200, 2, 4), ref.reshape(200, 2, 4))
    assert n_floor == 1 and err[3] == pytest.approx(0.25)
    out[5, 0] = np.nan
    assert R.worst(R.row_errors(out, ref)[0]) == np.inf
    with pytest.raises(AssertionError):
        A.assert_floor_cap(3, 200)


def test_lstm_clips_per_workgroup_rule():
    f = R.lstm_clips_per_workgroup
    assert [f(128, 2, 256), f(255, 2, 256), f(257, 2, 256)] == [1, 2, 4]
    assert [f(256, 1, 256), f(257, 1, 256), f(513, 1, 256)] == [1, 2, 4]
    for n in (8, 64, 256, 304):                           # the cases of the GPU test, whatever the chip's CU count
        assert [f(n - 1, 2, n), f(n + 1, 2, n), f(n + 1, 1, n), f(2 * n + 1, 1, n)] == [2, 4, 2, 4]
        assert f(n // 2, 2, n) == 1 and f(n // 2, 1, n) == 1
    assert f(1, 1, 256) == 1 and f(1, 2, 1) == 4


def test_no_reference_of_the_gpu_tests_is_floored():
    """Gaussian inputs: no row, column or clip of any fp64 reference used by test_gpu_probe_kernels.py sits under the norm floor."""
    T = R.LSTM_T
    shapes = [(B, T, H, 0) for B, H in R.LSTM_FORCED_CASES] + [(R.LSTM_BOUNDARY_BT[0], R.LSTM_BOUNDARY_BT[1], H, 0) for H in R.LSTM_BOUNDARY_H]
    shapes += [(B, R.LSTM_RULE_TH[0], R.LSTM_RULE_TH[1], 0) for B in (255, 257, 513)]
    for B, T_, H, seed in shapes:
        xg, w, xgr, wr = R.lstm_inputs(B, T_, H, seed)
        for ref in (R.lstm_ref(xg, w, False), R.lstm_ref(xgr, wr, True)):
            assert R.clip_errors(ref, ref)[1] == 0, (B, T_, H)
    xg, w, xgr, wr = R.lstm_saturated_inputs(257, *R.LSTM_RULE_TH)
    assert R.clip_errors(R.lstm_ref(xg, w, False), R.lstm_ref(xg, w, False))[1] == 0
    for M, N, K in [(M, N, K) for M in R.DENSE_MN for N in R.DENSE_MN for K in R.DENSE_K] + [R.DENSE_LONG]:
        x, w, b, r = R.dense_inputs(M, N, K)
        for act in R.ACTS:
            ref = R.dense_ref(x, w, b, act, r)
            assert R.row_errors(ref, ref)[1] == 0 and R.col_errors(ref, ref)[1] == 0, (M, N, K, act)
    B, T, H, D = R.MHA_LONG
    qkv = A.random_case(B, T, H, D, "f32")
    for pad in (None, A.pad_mask(B, T)):
        ref = A.plain_attention_ref(qkv, B, T, H, D, key_pad=pad)
        assert A.segment_errors(ref, ref, H, D)[1] == 0
    for Cc in R.INTERP_C:
        for Tin, Tout in R.INTERP_T:
            x = torch.from_numpy(R.interp_input(Tin, Cc))
            ref = torch.nn.functional.interpolate(x.transpose(1, 2), size=Tout, mode="linear", align_corners=False).transpose(1, 2)
            assert R.row_errors(ref.numpy().reshape(2 * Tout, Cc), ref.numpy().reshape(2 * Tout, Cc))[1] == 0, (Cc, Tin, Tout)


def test_fully_masked_clip_is_nan_in_torch():
    """nn.MultiheadAttention in fp64 gives NaN for a clip whose keys are all masked: what mha_f32 has to give."""
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(8, 2, batch_first=True).double().train()      # (train mode, no dropout: the plain path, not the fused one)
    x = torch.randn(3, 5, 8, dtype=torch.float64)
    pad = torch.zeros(3, 5, dtype=torch.bool)
    pad[1] = True
    with torch.no_grad():
        out, _ = mha(x, x, x, key_padding_mask=pad)
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all()
