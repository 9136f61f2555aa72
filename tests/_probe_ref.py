"""References and error instruments of the probe-kernel tests (test_probe_ref_cpu.py, test_gpu_probe_kernels.py, tools/lstm_forced_lr.py).

  * ``lstm_ref`` / ``dense_ref``: the operation in NumPy.  In float64 they are the reference; in float32 they restate the kernel's arithmetic
    (a sequential sum over k, an fp32 cell / epilogue) and measure what fp32 alone costs against fp64 in one particular order.  A test's bar
    is a multiple of that measure on the SAME inputs; it never sees device output.
  * ``row_errors`` / ``col_errors`` / ``clip_errors``: one relative L2 error per row, column or clip instead of one norm over the whole
    array, with the floor rule of ``_attention_ref.segment_errors`` (2^-6 x the median norm; the tests cap the floored share at 1 %).
  * ``lstm_clips_per_workgroup``: lstm.hip's choice of clips per workgroup, restated.
  * the shapes and seeded inputs shared by the CPU test, the GPU tests and the LSTM child process.
"""
import numpy as np
import torch

ACTS = (None, "relu", "gelu", "tanh")
FACTOR = 4.0      # fp32 kernels against an fp32 restatement in another summation order: MHA_FACTOR of test_gpu_attention_local.py


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    one = x.dtype.type(1.0)
    return one / (one + np.exp(-x))


def lstm_ref(xg, w_hh_t, reverse=False, dtype=np.float64):
    """One direction of one nn.LSTM layer as lstm.hip takes it: ``xg [B, T, 4H]`` is the input half of the gates (biases included),
    ``w_hh_t [H, 4H]`` is W_hh transposed, gates in the order i, f, g, o; returns h ``[B, T, H]`` in ``dtype``.
    float64: the reference.  float32: h W_hh^T summed over k in sequence, then added to xg, and the cell, all in fp32."""
    xg = np.asarray(xg, dtype)
    w = np.asarray(w_hh_t, dtype)
    B, T, G = xg.shape
    H = G // 4
    assert w.shape == (H, 4 * H)
    h = np.zeros((B, H), dtype)
    c = np.zeros((B, H), dtype)
    out = np.empty((B, T, H), dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(T):
            t = T - 1 - s if reverse else s
            if dtype == np.float64:
                acc = h @ w
            else:
                acc = np.zeros((B, 4 * H), dtype)
                for k in range(H):
                    acc += h[:, k, None] * w[k][None, :]
            g = xg[:, t] + acc
            ig, fg, gg, og = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
            c = fg * c + ig * gg
            h = og * np.tanh(c)
            out[:, t] = h
    assert out.dtype == dtype
    return out


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def activation(y, act):
    """None / "relu" / "gelu" (erf form) / "tanh" in ``y``'s own precision; a NaN stays a NaN under each of them."""
    t = y.dtype.type
    if act in (None, "none"):
        return y
    with np.errstate(invalid="ignore"):
        if act == "relu":
            return np.maximum(y, t(0.0))
        if act == "gelu":
            return t(0.5) * y * (t(1.0) + _erf(y * t(0.70710678118654752440)))
        if act == "tanh":
            return np.tanh(y)
    raise ValueError(act)


def dense_ref(x, w, bias=None, act=None, resid=None, dtype=np.float64):
    """``act(x @ w.T + bias) (+ resid)``: x ``[M, K]``, w ``[N, K]``.  float64: the reference.  float32: the sum over k accumulated in
    sequence (``acc += x[:, k] w[:, k]``: one chain per output, like the kernel's; not a BLAS call, whose blocked sums are more accurate
    than a chain), bias, activation and residual in fp32."""
    x = np.asarray(x, dtype)
    w = np.asarray(w, dtype)
    M, K = x.shape
    N = w.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == np.float64:
            acc = x @ w.T
        else:
            acc = np.zeros((M, N), dtype)
            for k in range(K):
                acc += x[:, k, None] * w[None, :, k]
        if bias is not None:
            acc = acc + np.asarray(bias, dtype)[None, :]
        y = activation(acc, act)
        if resid is not None:
            y = y + np.asarray(resid, dtype)
    assert y.dtype == dtype
    return y


# ---------------------------------------------------------------------------------------------------------------------------------
# instruments
# ---------------------------------------------------------------------------------------------------------------------------------
def _segment_errors(out, ref):
    """``out`` / ``ref`` as [segments, values]: (err per segment, number of floored segments)."""
    norm = np.linalg.norm(ref, axis=-1)
    floor = 2.0 ** -6 * float(np.median(norm))
    err = np.linalg.norm(out - ref, axis=-1) / np.maximum(norm, floor)
    return err, int((norm < floor).sum())


def row_errors(out, ref):
    """``(err [M], n_floor)`` of 2-D arrays: ``||out[m] - ref[m]|| / max(||ref[m]||, 2^-6 median row norm)``."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.ndim == 2 and out.shape == ref.shape
    return _segment_errors(out, ref)


def col_errors(out, ref):
    """The same per column."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.ndim == 2 and out.shape == ref.shape
    return _segment_errors(out.T, ref.T)


def clip_errors(out, ref):
    """The same per clip of ``[B, T, W]`` arrays."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.ndim == 3 and out.shape == ref.shape
    return _segment_errors(out.reshape(out.shape[0], -1), ref.reshape(ref.shape[0], -1))


def worst(err):
    """The largest error; a NaN anywhere counts as the worst."""
    return float(np.where(np.isnan(err), np.inf, err).max())


def lstm_clips_per_workgroup(B, dirs, n_cu):
    """lstm.hip's lstm_launch: four clips per workgroup, halved for as long as the workgroups of the smaller tile still fit the CUs."""
    lr = 4
    while lr > 1 and ((B + lr // 2 - 1) // (lr // 2)) * dirs <= n_cu:
        lr >>= 1
    return lr


# ---------------------------------------------------------------------------------------------------------------------------------
# shared shapes and inputs
# ---------------------------------------------------------------------------------------------------------------------------------
LSTM_T = 6
LSTM_FORCED_CASES = ((5, 256), (6, 300), (7, 512), (5, 1024), (7, 37), (5, 1))      # (B, H): remainders 1, 2, 3 against four clips; KS 4, 3, 2, 1
LSTM_GUARD_CLIPS = 4
LSTM_BOUNDARY_H = (256, 257, 341, 342, 512, 513, 1024)
LSTM_BOUNDARY_BT = (3, 3)
LSTM_RULE_TH = (4, 64)
DENSE_MN = (127, 128, 129)
DENSE_K = (4, 16, 20, 36, 17)
DENSE_LONG = (257, 130, 4100)
INTERP_C = (257, 768)
INTERP_T = ((40, 24), (1, 5), (5, 1), (1496, 496))      # (Tin, Tout)
MHA_LONG = (1, 2048, 2, 4)                              # B, T, H, head width: the kernel without the matrix core at its longest


def interp_input(Tin, Cc):
    """Gaussian ``[2, Tin, Cc]`` fp32."""
    from avex_amd import synth
    return synth.normal(f"itpw{Tin}_{Cc}", (2, Tin, Cc), 1.0)


def lstm_inputs(B, T, H, seed=0, scale=1.0):
    """Gaussian (xg, w_hh_t, xg_rev, w_hh_t_rev) fp32; the recurrent weights at nn.LSTM's H^-1/2 scale."""
    rng = np.random.default_rng([seed, B, T, H])
    xg, xgr = [(scale * rng.standard_normal((B, T, 4 * H))).astype(np.float32) for _ in range(2)]
    w, wr = [(rng.standard_normal((H, 4 * H)) * H ** -0.5).astype(np.float32) for _ in range(2)]
    return xg, w, xgr, wr


def lstm_saturated_inputs(B, T, H, seed=0):
    """The same with xg stretched so that its largest magnitude is 60: most gates saturated, on both sides."""
    xg, w, xgr, wr = lstm_inputs(B, T, H, seed)
    return (xg * np.float32(60.0 / np.abs(xg).max()), w, xgr * np.float32(60.0 / np.abs(xgr).max()), wr)


def lstm_refs(xg, w, xgr, wr):
    """(fp64 reference [B, T, 2H], fp32 restatement [B, T, 2H]): forward in the first H columns, reverse in the rest."""
    r64 = np.concatenate([lstm_ref(xg, w, False, np.float64), lstm_ref(xgr, wr, True, np.float64)], axis=-1)
    r32 = np.concatenate([lstm_ref(xg, w, False, np.float32), lstm_ref(xgr, wr, True, np.float32)], axis=-1)
    return r64, r32


def lstm_bar(r64, r32):
    """``(bar, n_floor, n_segments)``: FACTOR x the restatement's worst clip, over the clips of both directions of one case."""
    H = r64.shape[-1] // 2
    worst_e, n_floor, n = 0.0, 0, 0
    for sl in (slice(0, H), slice(H, 2 * H)):
        e, nf = clip_errors(r32[..., sl], r64[..., sl])
        worst_e, n_floor, n = max(worst_e, worst(e)), n_floor + nf, n + e.size
    return FACTOR * worst_e, n_floor, n


def dense_inputs(M, N, K, seed=0):
    """Gaussian (x [M, K], w [N, K] at K^-1/2, bias [N], resid [M, N]) fp32."""
    rng = np.random.default_rng([seed, M, N, K])
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) * K ** -0.5).astype(np.float32)
    return x, w, rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)


def dense_bars(x, w, b, act, r):
    """``(fp64 reference, row bar, column bar, floored, segments)`` of one dense case."""
    r64 = dense_ref(x, w, b, act, r, np.float64)
    r32 = dense_ref(x, w, b, act, r, np.float32)
    er, nr = row_errors(r32, r64)
    ec, nc = col_errors(r32, r64)
    return r64, FACTOR * worst(er), FACTOR * worst(ec), nr + nc, er.size + ec.size
