"""Attention references and the two instruments of the per-row attention tests (test_attention_cpu.py, test_gpu_attention_local.py).

  * fp64 references of the gated relative-position-bias attention and of plain multi-head attention (moved here from test_gpu_kernels.py);
  * ``segment_errors``: the error of every (clip, token, head) output segment on its own, instead of one norm over the whole output;
  * ``emulate``: the fp64 computation with the kernels' documented operand-type roundings and nothing else -- the measure of what a
    correct kernel may differ from fp64 by.  It never sees device output;
  * ``selector_case``: inputs for which every query attends to exactly one chosen key, so that "query i read key j and value row j"
    is asserted element by element;
  * ``range_case``: scores that start deep below zero, for the rarely entered branches of the deferred softmax reference.
"""
import math

import numpy as np

from _util import round_half
from oracle import beats_oracle as O

LOG2E = 1.4426950408889634
GLOBAL_BARS = {"f16": 1.5e-3, "bf16": 1.2e-2}      # the whole-output rel-L2 bars of test_gpu_kernels.py


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def attention_ref(qkv, B, T, H, table, gw, gb, ga, key_pad=None):
    E = H * 64
    q, k, v = [qkv[:, i * E:(i + 1) * E].reshape(B, T, H, 64).transpose(0, 2, 1, 3).astype(np.float64) for i in range(3)]
    s = q @ k.transpose(0, 1, 3, 2) * 0.125
    if table is not None:
        bias = O.position_bias(table, T, table.shape[0], 800 if table.shape[0] == 320 else 64).astype(np.float64)
        if gw is not None:
            g8 = q @ gw.T.astype(np.float64) + gb
            g2 = g8.reshape(B, H, T, 2, 4).sum(-1)
            sg = 1.0 / (1.0 + np.exp(-g2))
            gate = sg[..., 0:1] * (sg[..., 1:2] * ga.reshape(1, H, 1, 1) - 1.0) + 2.0
            s = s + gate * bias[None]
        else:
            s = s + bias[None]
    if key_pad is not None:
        s = np.where(key_pad[:, None, None, :], -np.inf, s)
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    o = (e / e.sum(-1, keepdims=True)) @ v
    return o.transpose(0, 2, 1, 3).reshape(B * T, E)


def plain_attention_ref(qkv, B, T, H, D, key_pad=None):
    E = H * D
    q, k, v = [qkv[:, i * E:(i + 1) * E].reshape(B, T, H, D).transpose(0, 2, 1, 3).astype(np.float64) for i in range(3)]
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(D)
    if key_pad is not None:
        s = np.where(key_pad[:, None, None, :], -np.inf, s)
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    o = (e / e.sum(-1, keepdims=True)) @ v
    return o.transpose(0, 2, 1, 3).reshape(B * T, E)


def toeplitz(table, T, nb, md):
    from avex_amd import kernels as K
    H = table.shape[1]
    tab = np.empty((H, 2 * T - 1), np.float32)
    for r in range(2 * T - 1):
        tab[:, r] = table[K.rel_bucket(r - (T - 1), nb, md)]
    return tab


def scores(qkv, B, T, H, D, table=None, gw=None, gb=None, ga=None):
    """The fp64 scores ``[B, H, T, T]`` (natural units, gate * bias included, no key mask) of either reference above."""
    E = H * D
    q, k = [qkv[:, i * E:(i + 1) * E].reshape(B, T, H, D).transpose(0, 2, 1, 3).astype(np.float64) for i in range(2)]
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(D)
    if table is not None:
        bias = O.position_bias(table, T, table.shape[0], 800 if table.shape[0] == 320 else 64).astype(np.float64)
        gate = 1.0
        if gw is not None:
            g2 = (q @ gw.T.astype(np.float64) + gb).reshape(B, H, T, 2, 4).sum(-1)
            sg = 1.0 / (1.0 + np.exp(-g2))
            gate = sg[..., 0:1] * (sg[..., 1:2] * ga.reshape(1, H, 1, 1) - 1.0) + 2.0
        s = s + gate * bias[None]
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# instrument 1: the error of each output segment
# ---------------------------------------------------------------------------------------------------------------------------------
def segment_errors(out, ref, H, D):
    """``(err, n_floor)``: ``err[r, h] = ||out - ref||_2 / max(||ref||_2, floor)`` over the D values of row r (clip * token), head h.
    The floor is 2^-6 x the median segment norm of ``ref``: a near-zero segment does not divide noise by nothing.  ``n_floor`` counts the
    segments whose norm was raised to the floor; a test lets at most 1 % of them be (``assert_floor_cap``)."""
    out = np.asarray(out, np.float64).reshape(-1, H, D)
    ref = np.asarray(ref, np.float64).reshape(-1, H, D)
    norm = np.linalg.norm(ref, axis=-1)
    floor = 2.0 ** -6 * float(np.median(norm))
    err = np.linalg.norm(out - ref, axis=-1) / np.maximum(norm, floor)
    return err, int((norm < floor).sum())


def assert_floor_cap(n_floor, n_segments):
    assert n_floor * 100 <= n_segments, f"{n_floor} of {n_segments} reference segments sit under the norm floor (cap: 1 %)"


def worst_segment(err):
    """``(value, (row, head))`` of the largest segment error; a NaN anywhere counts as the worst."""
    e = np.where(np.isnan(err), np.inf, err)
    r, h = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[r, h]), (int(r), int(h))


# ---------------------------------------------------------------------------------------------------------------------------------
# instrument 1's yardstick: fp64 with the kernels' operand-type roundings
# ---------------------------------------------------------------------------------------------------------------------------------
# Which roundings each kernel documents (read off its source; the variants differ):
#   attention.hip variant 1, attention_hd.hip: the query enters the MFMA as stored, the score scale is an fp32 multiply behind it; online
#       softmax over 32-key tiles: P is rounded against the running maximum up to and including its tile   -> round_q = False, "running_max"
#   attention.hip variant 2: the query fragment is multiplied by (T)(log2(e) / 8) in the operand type (two roundings: the constant and the
#       product); the gate is computed BEFORE that, from the stored query; deferred reference per 32-query tile -> round_q = True, "deferred32"
#   attention16.hip (variant 3): the same scaled fragment, and the gate's two dot products are taken from it on the matrix pipe (weights
#       times 8 ln 2, split hi + lo: fp32-level); deferred reference per 16-query block   -> round_q = True, gate_scaled_q = True, "deferred16"
#   the tail kernel of attention.hip (the rows beyond 512 of a bias-free clip): stored query, P against the row maximum  -> ``tail_rows``
#   every kernel: P rounded to the operand type in front of P V, the row sum over the unrounded P, the output rounded on its store.
# The reference P is rounded against is part of the rounding: 2^(s - m) is a power of two at the row's maximum only when m IS that maximum
# (one key, or a selector row: P = 1 exactly), and against a reference 2^12 above a score an f16 P is subnormal.  ``p_references``
# restates how each kernel picks it.
KERNEL_ROUNDINGS = {
    "1": dict(round_q=False, gate_scaled_q=False, p_reference="running_max"),
    "2": dict(round_q=True, gate_scaled_q=False, p_reference="deferred32"),
    "3": dict(round_q=True, gate_scaled_q=True, p_reference="deferred16"),
    "hd": dict(round_q=False, gate_scaled_q=False, p_reference="running_max"),
}
DEFER_THR, DEFER_HI, DEFER_LO = 8.0, 4096.0, 2.0 ** -6      # A2_THR / A3_THR, A3_SUM_HI, A3_SUM_LO


def p_references(s2, scheme):
    """``[B, H, T, ceil(T / 32)]``: the reference (base 2) each row's P is rounded against in each 32-key tile; ``s2`` = base-2 scores
    ``[B, H, T, T]`` with -inf on masked keys.
      row_max      the row's maximum, in every tile;
      running_max  the maximum up to and including the tile (variant 1, attention_hd.hip; 0 while every key so far is masked);
      deferred16   attention16.hip: a row starts without a reference and computes against 0.  After a tile's exponentials each lane holds
                   the sum of its 8 keys (keys 16 kb + 4 g + 0..3 of the tile, lane group g); a 16-query block is redone when ANY of its
                   lanes has a sum not below 2^12, or has a sum below 2^-6 in a row without a reference.  In a redone block a row without a
                   reference takes the tile's maximum (unless it is -inf) and a row with one moves it when the tile's maximum is more than
                   2^8 above; in a block that is not redone every row keeps what it has, 0 included, as its reference;
      deferred32   attention.hip variant 2: the same per 32-query tile with lanes of 16 keys (8 a + 4 hh + 0..3); a tile is redone when any
                   of its rows has no reference yet (so: always at first), or a lane's sum is not below 2^12."""
    B, H, T, _ = s2.shape
    nt = (T + 31) // 32
    sp = np.full((B, H, T, nt * 32), -np.inf)
    sp[..., :T] = s2
    sp = sp.reshape(B, H, T, nt, 32)
    tmax = sp.max(-1)
    if scheme == "row_max":
        return np.broadcast_to(tmax.max(-1, keepdims=True), tmax.shape).copy()
    if scheme == "running_max":
        run = np.maximum.accumulate(tmax, axis=-1)
        return np.where(np.isfinite(run), run, 0.0)
    assert scheme in ("deferred16", "deferred32")
    qb = 16 if scheme == "deferred16" else 32
    nqb = (T + qb - 1) // qb
    m = np.zeros((B, H, T))
    has = np.zeros((B, H, T), bool)
    ref = np.empty((B, H, T, nt))
    for kt in range(nt):
        S = sp[..., kt, :] - m[..., None]
        pt = np.exp2(S)
        if qb == 16:
            ls = pt.reshape(B, H, T, 2, 4, 4).sum((-3, -1))
            bad = (~(ls < DEFER_HI) | (~(ls >= DEFER_LO) & ~has[..., None])).any(-1)
        else:
            ls = pt.reshape(B, H, T, 4, 2, 4).sum((-3, -1))
            bad = (~(ls < DEFER_HI)).any(-1) | ~has
        blk = np.zeros((B, H, nqb * qb), bool)
        blk[..., :T] = bad
        redo = np.repeat(blk.reshape(B, H, nqb, qb).any(-1), qb, axis=-1)[..., :T]
        mx = S.max(-1)
        need = redo & np.where(has, mx > DEFER_THR, mx != -np.inf)
        m = m + np.where(need, mx, 0.0)
        has = has | need | ~redo
        ref[..., kt] = m
    return ref


def emulate(qkv, B, T, H, D, dtype, table=None, gw=None, gb=None, ga=None, key_pad=None, round_q=True, gate_scaled_q=False,
            p_reference="row_max", tail_rows=None, p_hook=None):
    """``[B*T, H*D]`` fp64: softmax(q k^T / sqrt(D) + gate * bias [+ mask]) v on operands already rounded to ``dtype``, with
      * Q scaled by log2(e) / sqrt(D) rounded to the operand type and the product rounded again (``round_q``), the scale applied in fp64
        otherwise;
      * the gate from the stored query, or from the scaled fragment (``gate_scaled_q``);
      * P rounded to the operand type in front of P V, against ``p_reference`` (see ``p_references``); the row sum over the unrounded P;
      * the output rounded to the operand type;
      * ``tail_rows`` (one bool per query row): these rows as the tail kernel computes them -- stored query, P against the row maximum.
    ``p_hook(p)`` may change the unrounded P ``[B, H, T, T]`` (relative to the row maximum) in place: the synthetic defects of
    test_attention_cpu.py."""
    E = H * D
    q, k, v = [qkv[:, i * E:(i + 1) * E].reshape(B, T, H, D).transpose(0, 2, 1, 3).astype(np.float64) for i in range(3)]
    cs = np.float32(np.float32(LOG2E) / np.float32(math.sqrt(D)))
    q2 = q * (LOG2E / math.sqrt(D))
    tail = np.zeros(T, bool) if tail_rows is None else np.asarray(tail_rows, bool)
    if round_q:
        csr = float(round_half(np.array([cs], np.float32), dtype)[0])
        q_rounded = round_half((q * csr).astype(np.float32), dtype).astype(np.float64)
        q2 = np.where(tail[None, None, :, None], q2, q_rounded)
    s2 = q2 @ k.transpose(0, 1, 3, 2)                      # base-2 scores
    if table is not None:
        bias = O.position_bias(table, T, table.shape[0], 800 if table.shape[0] == 320 else 64).astype(np.float64) * LOG2E
        gate = 1.0
        if gw is not None:
            w = gw.astype(np.float64)
            if gate_scaled_q:
                g8 = q2 @ (w.T * (math.sqrt(D) / LOG2E)) + gb
            else:
                g8 = q @ w.T + gb
            sg = 1.0 / (1.0 + np.exp(-g8.reshape(B, H, T, 2, 4).sum(-1)))
            gate = sg[..., 0:1] * (sg[..., 1:2] * ga.reshape(1, H, 1, 1) - 1.0) + 2.0
        s2 = s2 + gate * bias[None]
    if key_pad is not None:
        s2 = np.where(key_pad[:, None, None, :], -np.inf, s2)
    top = s2.max(-1, keepdims=True)
    p = np.exp2(s2 - top)
    if p_hook is not None:
        p_hook(p)
    l = p.sum(-1, keepdims=True)
    # P against its tile's reference, rounded, and brought back to the row maximum's scale (exact up to fp64)
    ref = p_references(s2, p_reference)
    if tail.any() and p_reference != "row_max":
        ref = np.where(tail[None, None, :, None], p_references(s2, "row_max"), ref)
    shift = np.repeat(top - ref, 32, axis=-1)[..., :T]      # >= 0 where P is not negligible: reference below the maximum
    pr = round_half((p * np.exp2(shift)).astype(np.float32), dtype).astype(np.float64) * np.exp2(-shift)
    o = (pr @ v) / l
    o = o.transpose(0, 2, 1, 3).reshape(B * T, E)
    return round_half(o.astype(np.float32), dtype).astype(np.float64)


def mha_f32_restatement(qkv, B, T, H, D, key_pad=None):
    """probe.hip's fp32 attention core restated in NumPy fp32 (scaled query, fp32 scores, exponentials, sums and products): what fp32
    arithmetic alone costs against fp64, in one particular summation order."""
    E = H * D
    q, k, v = [np.ascontiguousarray(qkv[:, i * E:(i + 1) * E].reshape(B, T, H, D).transpose(0, 2, 1, 3), np.float32) for i in range(3)]
    s = (q * np.float32(1.0 / np.sqrt(np.float32(D)))) @ k.transpose(0, 1, 3, 2)
    if key_pad is not None:
        s = np.where(key_pad[:, None, None, :], np.float32(-np.inf), s)
    e = np.exp(s - s.max(-1, keepdims=True), dtype=np.float32)
    o = (e @ v) * (np.float32(1.0) / e.sum(-1, keepdims=True, dtype=np.float32))
    return o.transpose(0, 2, 1, 3).reshape(B * T, E).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def pad_mask(B, T):
    """The key mask of the parity tests: clip 0 with a padded FIRST key tile, clip 1 with a padded tail that covers whole key tiles, and
    (three clips or more) clip 2 with ONE unpadded key.  None for a single token (an all-masked clip is another test's business)."""
    if T < 2:
        return None
    pad = np.zeros((B, T), bool)
    pad[0, :min(32, T - 1)] = True
    if B > 1:
        pad[1, max(1, T // 3):] = True
    if B > 2:
        pad[2, :] = True
        pad[2, (2 * T) // 3] = False
    return pad


def gate_params(seed=0):
    rng = np.random.default_rng(1000 + seed)
    gw = (0.1 * rng.standard_normal((8, 64))).astype(np.float32)
    gb = (0.1 * rng.standard_normal(8)).astype(np.float32)
    return gw, gb


def head_params(H, seed=0, table_std=0.5, table_clip=None):
    """(bias table [320, H], per-head gate scale ga [H])."""
    rng = np.random.default_rng(2000 + seed)
    table = (table_std * rng.standard_normal((320, H))).astype(np.float32)
    if table_clip is not None:
        table = np.clip(table, -table_clip, table_clip)
    ga = (1.0 + 0.2 * rng.standard_normal(H)).astype(np.float32)
    return table, ga


def round_to(x, dtype):
    """fp32 values rounded to the operand type ("f32": as they are)."""
    x = np.ascontiguousarray(x, np.float32)
    return x if dtype == "f32" else round_half(x, dtype)


def random_case(B, T, H, D, dtype, seed=0):
    """Gaussian q | k | v rows ``[B*T, 3*H*D]`` rounded to the operand type."""
    rng = np.random.default_rng([seed, B, T, H, D])
    return round_to(rng.standard_normal((B * T, 3 * H * D)), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# instrument 2: the selector
# ---------------------------------------------------------------------------------------------------------------------------------
# Factors (q, k) of the +-1 codes: exactly representable in f16 and bf16, target score q k sqrt(D) <= 48 (natural units).
SELECTOR_FACTORS = {32: (4.0, 2.0), 48: (3.0, 2.0), 64: (3.0, 2.0), 96: (2.0, 2.0), 128: (2.0, 2.0)}
SELECTOR_TABLE_CLIP = 0.7      # |gate * bias| <= 2.7 * 0.7 < 2 (gate = ga (gb a - 1) + 2 < 2.7 for a < 1.7): 48 + 2 <= 50
SELECTOR_DOMINATION = 2.0 ** -13
SELECTOR_SCORE_CAP = 50.0


def _codes(n, D, max_dot, rng):
    """n rows of +-1 in D columns, picked greedily: a candidate is kept when its dot product with every kept row is at most max_dot."""
    kept = np.empty((n, D), np.float64)
    m = 0
    for _ in range(400):
        cand = rng.integers(0, 2, size=(4 * n, D)).astype(np.float64) * 2.0 - 1.0
        for c in cand:
            if m == 0 or (kept[:m] @ c).max() <= max_dot:
                kept[m] = c
                m += 1
                if m == n:
                    return kept
    raise AssertionError(f"no {n} codes of width {D} with mutual dot products <= {max_dot}")


def selector_case(B, T, H, D, dtype, pad=None, bias=None, seed=0):
    """Inputs for which query i of clip b, head h attends to exactly one unpadded key pi[b, h, i], and pi is not the identity.

    Key j of a (clip, head) carries a +-1 code times ``SELECTOR_FACTORS[D][1]``, query i the code of its target times ``[0]``; the codes are
    picked so that an off-target score sits at least ln(T) + 19 (+ twice the bias range) below the target's: every other key together
    weighs less than 2^-27 -- far inside the asserted condition, so that the off-target rows stay under the selector bound's slack even
    for fp32.  V is uniform in +-[0.5, 1.5], rounded: no element near zero, so a relative bound per element means something.
    With ``pad`` ([B, T] bool), padded keys carry the code of some query's target (and their own V row): a kernel that forgets the mask for
    one key averages two rows.  ``bias`` = dict(table=, gw=, gb=, ga=) (gw / gb / ga may be None) adds the gated position bias.

    Asserted here, in fp64, gate * bias included: sum over j != pi(i) of exp(s_ij - s_i,pi(i)) <= 2^-13 for every row, and |s| <= 50.
    Returns ``(qkv [B*T, 3*H*D] fp32, pi [B, H, T], info)``."""
    assert T >= 2, "a selector needs a key other than the query's own"
    rng = np.random.default_rng([seed, B, T, H, D, 7])
    qf, kf = SELECTOR_FACTORS[D]
    target = qf * kf * math.sqrt(D)
    brange = 0.0
    if bias is not None:
        brange = 2.7 * float(np.abs(bias["table"]).max()) if bias.get("gw") is not None else float(np.abs(bias["table"]).max())
    gap = math.log(T) + 19.0 + 2.0 * brange
    max_dot = int(math.floor(D * (1.0 - gap / target) / 2.0)) * 2          # dots of +-1 rows of even width are even
    assert max_dot >= 0, (D, T, gap, target)
    base = _codes(T, D, max_dot, rng)
    q = np.empty((B, T, H, D), np.float64); k = np.empty((B, T, H, D), np.float64)
    pi = np.empty((B, H, T), np.int64)
    for b in range(B):
        live = np.flatnonzero(~pad[b]) if pad is not None else np.arange(T)
        dead = np.flatnonzero(pad[b]) if pad is not None else np.zeros(0, np.int64)
        assert live.size >= 1
        for h in range(H):
            code = base[rng.permutation(T)] * (rng.integers(0, 2, size=D) * 2.0 - 1.0)      # another key order and column signs per (clip, head)
            order = rng.permutation(live)
            t = order[np.arange(T) % live.size]
            if live.size > 1:
                same = t == np.arange(T)
                t[same] = order[(np.flatnonzero(same) + 1) % live.size]
            pi[b, h] = t
            if dead.size:                                   # padded keys repeat the codes of targets in use
                code[dead] = code[t[rng.integers(0, T, size=dead.size)]]
            k[b, :, h] = kf * code
            q[b, :, h] = qf * code[t]
    sign = rng.integers(0, 2, size=(B, T, H, D)) * 2.0 - 1.0
    v = sign * (0.5 + rng.random((B, T, H, D)))
    qkv = np.concatenate([x.reshape(B * T, H * D) for x in (q, k, v)], axis=1).astype(np.float32)
    qkv = round_to(qkv, dtype)
    assert np.array_equal(qkv[:, :2 * H * D], np.concatenate([q.reshape(B * T, -1), k.reshape(B * T, -1)], 1)), "codes must be exact in the operand type"

    kw = {} if bias is None else dict(table=bias["table"], gw=bias.get("gw"), gb=bias.get("gb"), ga=bias.get("ga"))
    s = scores(qkv, B, T, H, D, **kw)
    assert np.abs(s).max() <= SELECTOR_SCORE_CAP, np.abs(s).max()
    if pad is not None:
        s = np.where(pad[:, None, None, :], -np.inf, s)
    st = np.take_along_axis(s, pi[..., None], axis=-1)
    assert np.isfinite(st).all(), "a target is padded"
    w = np.exp(s - st)
    np.put_along_axis(w, pi[..., None], 0.0, axis=-1)
    eps = float(w.sum(-1).max())
    assert eps <= SELECTOR_DOMINATION, eps
    not_identity = (pi != np.arange(T)[None, None, :])
    assert not_identity.any() and (pad is not None or not_identity.all())
    return qkv, pi, dict(eps=eps, max_score=float(np.abs(s[np.isfinite(s)]).max()), max_dot=max_dot)


def selector_expected(qkv, pi, B, T, H, D):
    """``[B*T, H*D]``: row i of (clip, head) is V[pi(i)]."""
    E = H * D
    v = qkv[:, 2 * E:].reshape(B, T, H, D).astype(np.float64)
    out = np.empty((B, T, H, D), np.float64)
    for b in range(B):
        for h in range(H):
            out[b, :, h] = v[b, pi[b, h], h]
    return out.reshape(B * T, E)


def selector_mismatch(out, qkv, pi, B, T, H, D, rel):
    """None when every output element is within ``rel * |v|`` of V[pi(i)]; else a message naming the first failing (clip, head, query), its
    target and the key whose V row the output is closest to."""
    exp = selector_expected(qkv, pi, B, T, H, D).reshape(B, T, H, D)
    got = np.asarray(out, np.float64).reshape(B, T, H, D)
    bad = ~(np.abs(got - exp) <= rel * np.abs(exp))      # (a NaN fails)
    if not bad.any():
        return None
    b, i, h = [int(x) for x in np.argwhere(bad.any(-1))[0]]
    v = qkv[:, 2 * H * D:].reshape(B, T, H, D).astype(np.float64)[b, :, h]
    near = int(np.argmin(np.linalg.norm(v - got[b, i, h][None], axis=-1))) if np.isfinite(got[b, i, h]).all() else -1
    worst = float(np.nanmax(np.abs(got[b, i, h] - exp[b, i, h]) / np.abs(exp[b, i, h])))
    return (f"{int(bad.any(-1).sum())} of {B * T * H} segments off; first: clip {b} head {h} query {i} should read key {int(pi[b, h, i])}, "
            f"its output is closest to the V row of key {near} (worst element off by {worst:.3e} of |v|, bound {rel:.3e})")


# ---------------------------------------------------------------------------------------------------------------------------------
# range paths: scores far below zero
# ---------------------------------------------------------------------------------------------------------------------------------
RANGE_PATTERNS = ("downward_start", "flat_minus_40", "mixed_rows", "masked_then_deep")


def range_case(pattern, B, T, H, D, dtype, seed=0):
    """``(qkv, pad or None)`` with a constant on q and a ramp on k, as test_attention_large_logits builds its scores:
      downward_start    every query: scores near -60 on the first key tiles rising to 0 at the last keys -- a streamed kernel's first
                        reference is NEGATIVE (the first tile's numerators would all be subnormal against 0), then it moves;
      flat_minus_40     every score in -40 +- 1: a negative reference that never moves;
      mixed_rows        odd queries gaussian (|s| of a few units), even queries as in downward_start: the lanes of one 16-query block
                        disagree about moving the reference while all of them hold one;
      masked_then_deep  downward_start behind a fully padded first key tile: the first tile leaves the row without a reference, the
                        second sets a negative one.
    The ranges are asserted by ``assert_range_case`` on the fp64 scores."""
    assert pattern in RANGE_PATTERNS
    rng = np.random.default_rng([seed, B, T, H, D, RANGE_PATTERNS.index(pattern)])
    ones = np.ones(D)
    r = 1.0 - np.arange(T) / max(T - 1, 1)                 # 1 at key 0, 0 at the last key
    g = rng.standard_normal((B, T, H, D))
    v = rng.standard_normal((B, T, H, D))
    if pattern == "flat_minus_40":
        # q = 3, k = -(40 sqrt(D) / 3 D) (1 + 0.02 g): s = -40 (1 + 0.02 mean(g)), within +- 0.4 for D >= 64
        q = np.broadcast_to(3.0 * ones, (B, T, H, D)).copy()
        k = -(40.0 * math.sqrt(D) / (3.0 * D)) * (1.0 + 0.02 * g)
    else:
        # k = -kc r(j) + 0.5 g with 3 D kc / sqrt(D) = 60;  q = 3 (ramp rows): s = -60 r(j) + 1.5 N(0, 1);
        # q = 2 (gaussian - its mean over d) (gaussian rows): blind to the ramp, s ~ N(0, 1)
        kc = 60.0 * math.sqrt(D) / (3.0 * D)
        k = -kc * r[None, :, None, None] * ones + 0.5 * g
        q = np.broadcast_to(3.0 * ones, (B, T, H, D)).copy()
        if pattern == "mixed_rows":
            n = rng.standard_normal((B, T, H, D))
            n = round_half((2.0 * n).astype(np.float32), dtype).astype(np.float64)
            # the mean is removed AFTER rounding, in steps the operand type holds exactly (multiples of 2^-6 for |x| < 8 in bf16):
            # what is left of the ramp in a gaussian row is then a few units at most
            n = n - np.round(n.mean(-1, keepdims=True) * 64.0) / 64.0
            q[:, 1::2] = n[:, 1::2]
    pad = None
    if pattern == "masked_then_deep":
        pad = np.zeros((B, T), bool)
        pad[:, :32] = True
    qkv = np.concatenate([x.reshape(B * T, H * D) for x in (q, k, v)], axis=1).astype(np.float32)
    return round_half(qkv, dtype), pad


def assert_range_case(pattern, qkv, B, T, H, D, table=None):
    s = scores(qkv, B, T, H, D, table=table)
    if pattern == "flat_minus_40":
        assert np.abs(s + 40.0).max() <= 1.0, np.abs(s + 40.0).max()
        return
    ramp = s[:, :, 0::2] if pattern == "mixed_rows" else s
    first = 64 if pattern == "masked_then_deep" else 32
    lo = ramp[..., first - 32:first]                        # the first unmasked key tile
    assert lo.max() < -40.0 and lo.min() > -75.0, (lo.min(), lo.max())
    assert np.abs(ramp[..., -32:]).max() < 15.0, np.abs(ramp[..., -32:]).max()
    assert ramp.max(-1).min() > -6.0                          # every ramp row ends near 0
    if pattern == "mixed_rows":
        assert np.abs(s[:, :, 1::2]).max() < 12.0, np.abs(s[:, :, 1::2]).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of test_gpu_attention_local.py (test_attention_cpu.py checks the instruments on every one of them)
# ---------------------------------------------------------------------------------------------------------------------------------
ENC_B, ENC_H = 3, 4
ENC_GRID = 3                                   # 12 (head, clip) items in runs of 4: every workgroup crosses a head seam mid-run
ENC_T_TABLE = (1, 17, 33, 257, 496, 512)       # gate + bias table + key mask, variants 1 / 2 / 3
ENC_T_PLAIN = ((499, 0), (513, 0), (544, 32), (544, 0))      # no table: (T, tail rows asked for; 0 = the default of 2)
ENC_LONG = ((545, 6), (1037, 5))               # (T, grid): (item, query block) units in runs of 3 (of 2 per item) and 5 (of 3 per item)
ENC_LONG_B = 2
HD_B, HD_H = 3, 4
HD_D = (32, 64, 96, 128)
HD_T = (37, 129, 300)
MHA_D = (32, 48, 64, 96, 128)                  # 48: the kernel without the matrix core
SEL_T_TABLE = (33, 257, 496, 512)
SEL_T_PLAIN = ((513, 0), (544, 32))
SEL_T_LONG = ((1037, 5),)
SEL_HD_T = (129, 300)
RANGE_B, RANGE_H, RANGE_T, RANGE_GRID = 2, 4, 496, 3
RANGE_TABLE_STD, RANGE_TABLE_CLIP = 0.15, 0.4  # keeps flat_minus_40 inside +- 1 with the table added


def tail_rows(T, asked):
    """Per query row: True where attention.hip's tail kernel computes it (the 1 .. 32 rows beyond 512 of a bias-free clip, when the last
    query block has at most ``asked`` rows; the library's default asks for 2)."""
    rem = T % 512
    on = T > 512 and 0 < rem <= (asked or 2) and rem <= 32
    rows = np.zeros(T, bool)
    if on:
        rows[T - rem:] = True
    return rows
