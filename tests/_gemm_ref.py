"""The epilogue of avexhip_gemm restated in fp64, in the order the kernels apply it (avex_amd/csrc/gemm.hip; include/avexhip.h):

    1. acc + bias            2. row_zero: masked rows become 0        3. raw tap
    4. + resid * alpha       5. activation code 0..5                  6. fp32 output
    7. * half_scale, rounded to the operand type                      8. n_store: only the leading columns exist
    9. LayerNorm of the rows of 6 (or of 7 with post_ln_round)        10. a_scale: A[m] *= a_scale[m // a_scale_rows], the fp32
                                                                          product rounded to the operand type, before the product

Plain torch on whatever device the inputs live on; every result is fp64.  tests/test_gemm_ref_cpu.py pins it against torch.nn.functional.
The per-row error measure of tests/test_gpu_gemm_args.py lives here too."""
import math

import torch

F16_ROW_TOL = {"f16": 2e-3, "bf16": 1.5e-2}      # one output row in the operand type against fp64 (test_gemm_folded_layernorm's last-row bound)
F32_ROW_TOL = 1e-5                               # one fp32 output row against fp64


def tdt(name):
    return torch.float16 if name in ("f16", torch.float16) else torch.bfloat16


def round_to(x, dtype):
    """fp64 / fp32 values as the operand type holds them (through fp32, like the kernels), back in fp64."""
    return x.to(torch.float32).to(tdt(dtype)).to(torch.float64)


def activation(x, code):
    """GemmArgs::gelu codes on an fp64 tensor: 0 none, 1 erf GELU, 2 SiLU, 3 ReLU, 4 tanh-form GELU, 5 tanh."""
    if code == 0:
        return x
    if code == 1:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if code == 2:
        return x / (1.0 + torch.exp(-x))
    if code == 3:
        return torch.clamp_min(x, 0.0)
    if code == 4:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if code == 5:
        return torch.tanh(x)
    raise ValueError(f"activation code {code}")


def scaled_rows(a, a_scale, a_scale_rows):
    """Step 10 with the kernels' own arithmetic: the fp32 product of a half row and its clip's scales, rounded to the operand type."""
    M, K = a.shape
    clip = torch.arange(M, device=a.device) // a_scale_rows
    return (a.float() * a_scale[clip, :K].float()).to(a.dtype)


def layer_norm(y, w, b, eps):
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    return (y - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def gemm_ref(a, w, dtype, *, bias=None, row_zero=None, resid=None, alpha=1.0, act=0, half_scale=0.0, n_store=0,
             a_scale=None, a_scale_rows=0, post_ln_w=None, post_ln_b=None, post_ln_eps=1e-5, post_ln_round=0):
    """a [M, K], w [N, K] in the operand type; resid fp32 or half, as wide as the stored columns.  Returns raw / f32 / half (and ln_f32 /
    ln_half with post_ln_w), fp64, n_store columns wide when that is set."""
    if a_scale is not None:
        a = scaled_rows(a, a_scale, a_scale_rows)
    N = w.shape[0]
    v = a.double() @ w.double().T
    if bias is not None:
        v = v + bias.double()
    if row_zero is not None:
        v = torch.where(row_zero.to(v.device).bool()[:, None], torch.zeros_like(v), v)
    ns = n_store if 0 < n_store < N else N
    v = v[:, :ns]
    out = {"raw": v}
    if resid is not None:
        v = resid.double()[:, :ns] * float(alpha) + v
    v = activation(v, act)
    out["f32"] = v
    scale = float(half_scale) if half_scale not in (0.0, 1.0) else 1.0
    out["half"] = round_to(v * scale, dtype)
    if post_ln_w is not None:
        y = round_to(v, dtype) if post_ln_round else v
        ln = layer_norm(y, post_ln_w, post_ln_b, post_ln_eps)
        out["ln_f32"] = ln
        out["ln_half"] = round_to(ln, dtype)
    return out


def row_errors(got, want):
    """rel-L2 of every row of `got` against `want` (fp64): one wrong row in thousands is one entry near 1, not a 1e-3 of the whole.
    A reference row that is exactly zero must be matched exactly (error 0 or inf)."""
    got, want = got.double(), want.double()
    num = (got - want).norm(dim=-1)
    den = want.norm(dim=-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def worst_row(got, want):
    err = row_errors(got, want)
    i = int(err.argmax())
    return float(err[i]), i
