"""The row kernels of avex_amd/csrc/elementwise.hip restated in NumPy: fp64 where a kernel is judged by its error, fp32 in the kernel's
own order where it is judged by its bits.  tests/test_rows_ref_cpu.py pins these against torch on the CPU; tests/test_gpu_rows.py
compares the kernels with them.  Nothing here calls the library."""
import numpy as np

F32_ULP = 2.0 ** -23
HALF_MANT = {"f16": 10, "bf16": 7}            # explicit mantissa bits
HALF_EMIN = {"f16": -14, "bf16": -126}        # exponent of the smallest normal number
HALF_MAX = {"f16": 65504.0, "bf16": 3.3895313892515355e38}


def layer_norm(x, w, b, eps):
    """Two-pass LayerNorm over the last axis in fp64 (mean, then centred variance, eps inside the square root)."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def row_rstd(x, eps):
    """1 / sqrt(var + eps) of every row, fp64 ``[..., 1]``."""
    x = np.asarray(x, np.float64)
    d = x - x.mean(-1, keepdims=True)
    return 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)


def layer_norm_pool(x, w, b, eps):
    """``[B, T, C]`` -> ``[B, C]``: the mean over tokens of the LayerNorm of every token, fp64."""
    return layer_norm(x, w, b, eps).mean(axis=1)


def glu_swish(y):
    """``[M, 2F]`` -> ``[M, F]``: ``a * g * sigmoid(g)`` with a = the first half of a row, g = the second, fp64.  The sigmoid is written so
    that no exponential overflows: 1 / (1 + e^-g) for g >= 0 and e^g / (1 + e^g) below."""
    y = np.asarray(y, np.float64)
    F = y.shape[-1] // 2
    a, g = y[..., :F], y[..., F:]
    with np.errstate(invalid="ignore", under="ignore"):      # (e^-65504 is 0, and inf * 0 is the NaN torch gives too)
        e = np.exp(-np.abs(g))
        sig = np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return a * (g * sig)


def row_sums(w):
    return np.asarray(w, np.float64).sum(axis=-1)


def toeplitz(table, lut, maxd, T):
    """``out[h][r] = table[lut[clamp(r - (T - 1), -maxd, maxd) + maxd]][h]``: ``[H, 2T - 1]`` in the table's own type (a gather, exact)."""
    table, lut = np.asarray(table), np.asarray(lut)
    d = np.clip(np.arange(2 * T - 1) - (T - 1), -maxd, maxd)
    return np.ascontiguousarray(table[lut[d + maxd]].T)


def mean_pool_f32(x):
    """mean_pool_kernel's own arithmetic, fp32, bit for bit: four token phases t % 4, each added in increasing t starting from +0, combined
    as (p0 + p1) + (p2 + p3) and divided by T.  ``[B, T, C]`` fp32 -> ``[B, C]`` fp32."""
    x = np.asarray(x, np.float32)
    B, T, C = x.shape
    p = np.zeros((4, B, C), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            p[t % 4] = p[t % 4] + x[:, t]
        tot = (p[0] + p[1]) + (p[2] + p[3])
        return (tot / np.float32(T)).astype(np.float32)


def max_pool(x):
    """``[B, T, C]`` -> ``[B, C]``: the maximum over tokens; a NaN in a column stays (numpy's max, like torch.max over a dimension)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(x).max(axis=1)


def lnr_fold(gamma, beta, bias, alpha):
    """(gamma * alpha, bias + alpha * beta) in fp64; alpha is taken as the fp32 number the kernel receives."""
    a = np.float64(np.float32(alpha))
    return np.asarray(gamma, np.float64) * a, np.asarray(bias, np.float64) + a * np.asarray(beta, np.float64)


def half_ulp(v, dtype):
    """The spacing of the operand type's numbers at |v| (fp64 array): 2^(e - mantissa bits) with e = floor(log2 |v|), never below the
    subnormal spacing."""
    v = np.abs(np.asarray(v, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    e = np.maximum(np.where(v > 0, e, HALF_EMIN[dtype]), HALF_EMIN[dtype])
    return np.exp2(e - HALF_MANT[dtype])


def f32_ulp(v):
    v = np.abs(np.asarray(v, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    e = np.maximum(np.where(v > 0, e, -126.0), -126.0)
    return np.exp2(e - 23)
