"""The instruments of test_gpu_attention_local.py, tested without a GPU: the per-segment measure sees defects the whole-output rel-L2 of
test_gpu_kernels.py does not, the selector inputs meet their conditions at every shape the GPU tests use, and no random-input case
leans on the segment-norm floor."""
import numpy as np
import pytest

import _attention_ref as A
from _util import rel_l2

DTYPES = ["f16", "bf16"]


# ---- the synthetic defects ------------------------------------------------------------------------------------------------------------
_DB, _DH, _DT, _DD = 2, 12, 496, 64      # the encoder's shape: about 1.2e4 (clip, token, head) segments


@pytest.fixture(scope="module", params=DTYPES)
def defect_base(request):
    dtype = request.param
    qkv = A.random_case(_DB, _DT, _DH, _DD, dtype)
    ref = A.plain_attention_ref(qkv, _DB, _DT, _DH, _DD)
    emu = A.emulate(qkv, _DB, _DT, _DH, _DD, dtype)
    err, n_floor = A.segment_errors(emu, ref, _DH, _DD)
    A.assert_floor_cap(n_floor, err.size)
    # the bar of the GPU tests (section a): twice the emulation's own worst segment
    return dict(dtype=dtype, qkv=qkv, ref=ref, bar=2.0 * A.worst_segment(err)[0], clean_global=rel_l2(emu, ref))


def _with_defect(base, hook):
    emu = A.emulate(base["qkv"], _DB, _DT, _DH, _DD, base["dtype"], p_hook=hook)
    err, _ = A.segment_errors(emu, base["ref"], _DH, _DD)
    return err.reshape(_DB, _DT, _DH), rel_l2(emu, base["ref"])


def test_rounding_alone_sits_well_under_the_global_bars(defect_base):
    assert defect_base["clean_global"] < 0.5 * A.GLOBAL_BARS[defect_base["dtype"]]
    assert defect_base["bar"] < 4.0 * A.GLOBAL_BARS[defect_base["dtype"]]      # the segment bar is of the same order, not a loose one


def test_one_key_dropped_for_one_query_block_passes_the_global_bar_and_fails_the_segment_bar(defect_base):
    """A mis-masked key at one tile edge: one key lost to the 16 queries of one block of one head.  The whole-output rel-L2 stays under
    the bars of test_gpu_kernels.py in both types; the worst segment exceeds the per-segment bar."""
    b, h, rows = 1, 5, slice(160, 176)

    def hook(p):      # a key of typical weight for these rows: the median one
        p[b, h, rows, int(np.argsort(p[b, h, rows].sum(0))[_DT // 2])] = 0.0
    err, glob = _with_defect(defect_base, hook)
    print(f"{defect_base['dtype']}: global {glob:.2e} (bar {A.GLOBAL_BARS[defect_base['dtype']]:.1e}), worst segment {err[b, rows, h].max():.2e} (bar {defect_base['bar']:.2e})")
    assert glob < A.GLOBAL_BARS[defect_base["dtype"]]
    assert err[b, rows, h].max() > defect_base["bar"]
    other = err.copy(); other[b, rows, h] = 0.0
    assert other.max() <= 0.5 * defect_base["bar"]      # and nowhere else


def test_one_key_dropped_for_a_whole_head_and_a_swapped_row_fail_the_segment_bar(defect_base):
    """One key lost to every row of one (clip, head) (a k-slot / key mismatch), and one row's P taken from its neighbour (one row's gate or
    bias run read from another row)."""
    b1, h1 = 0, 3
    b2, h2, i2 = 1, 7, 100

    def hook(p):
        p[b1, h1, :, int(np.argmax(p[b1, h1].sum(0)))] = 0.0      # (here the key that matters most to the head)
        p[b2, h2, i2] = p[b2, h2, i2 + 1]
    err, glob = _with_defect(defect_base, hook)
    print(f"{defect_base['dtype']}: global {glob:.2e}, dropped key: worst segment {err[b1, :, h1].max():.2e}; swapped row: {err[b2, i2, h2]:.2e} (bar {defect_base['bar']:.2e})")
    assert err[b1, :, h1].max() > 10.0 * defect_base["bar"]
    assert err[b2, i2, h2] > 10.0 * defect_base["bar"]


# ---- the selector inputs ----------------------------------------------------------------------------------------------------------------
def _selector_bias(H):
    table, ga = A.head_params(H, table_clip=A.SELECTOR_TABLE_CLIP)
    gw, gb = A.gate_params()
    return dict(table=table, gw=gw, gb=gb, ga=ga)


_SEL_ENC = [(A.ENC_B, T, True) for T in A.SEL_T_TABLE] + [(A.ENC_B, T, False) for T, _ in A.SEL_T_PLAIN] + [(A.ENC_LONG_B, T, True) for T, _ in A.SEL_T_LONG]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,table", _SEL_ENC)
def test_selector_case_meets_its_conditions_encoder_shapes(B, T, table, dtype):
    """selector_case asserts domination (<= 2^-13) and |s| <= 50 itself; here: at every shape of the GPU tests, with and without mask / bias."""
    H, D = A.ENC_H, 64
    qkv, pi, info = A.selector_case(B, T, H, D, dtype)
    assert info["eps"] <= A.SELECTOR_DOMINATION and info["max_score"] <= A.SELECTOR_SCORE_CAP
    pad = A.pad_mask(B, T)
    qkv, pi, info = A.selector_case(B, T, H, D, dtype, pad=pad, bias=_selector_bias(H) if table else None)
    assert info["eps"] <= A.SELECTOR_DOMINATION and info["max_score"] <= A.SELECTOR_SCORE_CAP
    assert not np.take_along_axis(np.broadcast_to(pad[:, None, :], pi.shape), pi, axis=-1).any()      # no target is a padded key
    # a padded key carries a target's code: forgetting its mask would change the output
    E = H * D
    k = qkv[:, E:2 * E].reshape(B, T, H, D)
    hit = 0
    for b in range(B):
        for j in np.flatnonzero(pad[b])[:8]:
            hit += int((k[b, ~pad[b], 0] == k[b, j, 0]).all(-1).any())
    assert hit > 0


@pytest.mark.parametrize("D", sorted(set(A.HD_D) | set(A.MHA_D)))
@pytest.mark.parametrize("T", A.SEL_HD_T)
def test_selector_case_meets_its_conditions_other_head_widths(D, T):
    for dtype in DTYPES + ["f32"]:
        for pad in (None, A.pad_mask(A.HD_B, T)):
            _, _, info = A.selector_case(A.HD_B, T, A.HD_H, D, dtype, pad=pad)
            assert info["eps"] <= A.SELECTOR_DOMINATION and info["max_score"] <= A.SELECTOR_SCORE_CAP
            # what the fp32 bound of the GPU test leans on: the off-target rows (|v| <= 1.5 against |v| >= 0.5) stay under one fp32 ulp
            assert 6.0 * info["eps"] < 2.0 ** -24


# ---- the floor cap ----------------------------------------------------------------------------------------------------------------------
def _floor_ok(ref, H, D):
    err, n_floor = A.segment_errors(ref, ref, H, D)
    A.assert_floor_cap(n_floor, err.size)
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_floor_cap_holds_for_the_encoder_cases(dtype):
    H = A.ENC_H
    gw, gb = A.gate_params()
    table, ga = A.head_params(H)
    for T in A.ENC_T_TABLE:
        qkv = A.random_case(A.ENC_B, T, H, 64, dtype)
        for pad in (None, A.pad_mask(A.ENC_B, T)):
            _floor_ok(A.attention_ref(qkv, A.ENC_B, T, H, table, gw, gb, ga, key_pad=pad), H, 64)
    for T in sorted({T for T, _ in A.ENC_T_PLAIN}):
        qkv = A.random_case(A.ENC_B, T, H, 64, dtype)
        for pad in (None, A.pad_mask(A.ENC_B, T)):
            _floor_ok(A.attention_ref(qkv, A.ENC_B, T, H, None, None, None, None, key_pad=pad), H, 64)
    for T, _ in A.ENC_LONG:
        qkv = A.random_case(A.ENC_LONG_B, T, H, 64, dtype)
        for pad in (None, A.pad_mask(A.ENC_LONG_B, T)):
            _floor_ok(A.attention_ref(qkv, A.ENC_LONG_B, T, H, table, gw, gb, ga, key_pad=pad), H, 64)


@pytest.mark.parametrize("dtype", DTYPES + ["f32"])
def test_floor_cap_holds_for_the_other_head_widths(dtype):
    for D in (A.MHA_D if dtype == "f32" else A.HD_D):
        for T in A.HD_T:
            qkv = A.random_case(A.HD_B, T, A.HD_H, D, dtype)
            for pad in (None, A.pad_mask(A.HD_B, T)):
                _floor_ok(A.plain_attention_ref(qkv, A.HD_B, T, A.HD_H, D, key_pad=pad), A.HD_H, D)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern", A.RANGE_PATTERNS)
def test_range_cases_have_the_intended_scores(pattern, dtype):
    B, H, T = A.RANGE_B, A.RANGE_H, A.RANGE_T
    table, _ = A.head_params(H, table_std=A.RANGE_TABLE_STD, table_clip=A.RANGE_TABLE_CLIP)
    for D in (64, 96) if pattern in A.RANGE_PATTERNS[:2] else (64,):
        qkv, pad = A.range_case(pattern, B, T, H, D, dtype)
        assert (pad is not None) == (pattern == "masked_then_deep")
        A.assert_range_case(pattern, qkv, B, T, H, D, table=table if D == 64 else None)
        ref = A.attention_ref(qkv, B, T, H, table, None, None, None, key_pad=pad) if D == 64 else A.plain_attention_ref(qkv, B, T, H, D, key_pad=pad)
        _floor_ok(ref, H, D)


def test_segment_errors_counts_the_floor():
    ref = np.ones((8, 2 * 4)); ref[0, :4] = 1e-9
    out = ref.copy(); out[0, :4] += 1e-3; out[3, 4:] *= 1.5
    err, n_floor = A.segment_errors(out, ref, 2, 4)
    assert err.shape == (8, 2) and n_floor == 1
    assert np.isclose(err[0, 0], 2e-3 / (2.0 ** -6 * 2.0)) and np.isclose(err[3, 1], 0.5) and err.sum() == err[0, 0] + err[3, 1]
    with pytest.raises(AssertionError):
        A.assert_floor_cap(2, 100)
