"""Plain fp64 NumPy restatements of the audio front ends (avex_amd/csrc/fbank.hip, melspec.hip, ingest.hip, posconv.hip), written from
what the kernels document and independent of their structure: every frame is transformed alone, every sum runs in fp64.

TEST INFRASTRUCTURE ONLY.  tests/test_frontend_ref_cpu.py pins each function against what the project already trusts (the fp32 oracles
under oracle/ and torch.stft); tests/test_gpu_frontends.py compares the kernels with them off the shipped models' settings.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
from scipy.special import erf as _erf

FBANK_NFFT = 512                      # the filterbank kernel's transform length, whatever the window length
MEL_LOG_EPS = float(np.float32(1e-6))  # the constant inside the mel front end's log, as the kernel holds it


# ------------------------------------------------------------------------------------------------------------------------
# kaldi filterbank (fbank.hip)
# ------------------------------------------------------------------------------------------------------------------------
def fbank_frames(T: int, win: int, hop: int) -> int:
    return 0 if T < win else 1 + (T - win) // hop


def fbank64(wav, *, win, hop, preemph, remove_dc, window, mel_fb, input_scale, clip_offset=None) -> np.ndarray:
    """Mel ENERGIES ``[B, frames, n_mels]`` (fp64): per clip ``(x - clip_offset) * input_scale``; frames of ``win`` samples every ``hop``
    (no padding, the tail is cut); per frame the mean is removed (``remove_dc``), then ``y[n] = x[n] - preemph * x[max(n - 1, 0)]``, the window,
    zero padding to 512 points, ``|rfft|^2`` and the ``[257, n_mels]`` bank."""
    x = np.asarray(wav, np.float64)
    if clip_offset is not None:
        x = x - np.asarray(clip_offset, np.float64).reshape(-1, 1)
    x = x * float(input_scale)
    B, T = x.shape
    mel_fb = np.asarray(mel_fb, np.float64)
    n = fbank_frames(T, win, hop)
    if n == 0:
        return np.zeros((B, 0, mel_fb.shape[1]))
    fr = x[:, np.arange(n)[:, None] * hop + np.arange(win)[None, :]]               # [B, n, win]
    with np.errstate(invalid="ignore", over="ignore"):                             # (a NaN / Inf sample on purpose)
        if remove_dc:
            fr = fr - fr.sum(axis=-1, keepdims=True) / win
        prev = np.concatenate([fr[..., :1], fr[..., :-1]], axis=-1)
        fr = (fr - float(preemph) * prev) * np.asarray(window, np.float64)
        spec = np.fft.rfft(fr, n=FBANK_NFFT, axis=-1)
        return (spec.real ** 2 + spec.imag ** 2) @ mel_fb


def fbank_log(energy, log_floor, norm_mean=0.0, norm_div=1.0) -> np.ndarray:
    """``(log(max(e, floor)) - mean) / div``; a NaN energy stays NaN (np.maximum propagates it)."""
    div = 1.0 if norm_div == 0 else float(np.float32(norm_div))
    with np.errstate(invalid="ignore"):
        return (np.log(np.maximum(energy, float(np.float32(log_floor)))) - float(np.float32(norm_mean))) / div


def fbank_pad(img, out_frames, norm_mean=0.0, norm_div=1.0) -> np.ndarray:
    """``FbankPlan.padded``: rows past the last frame hold the normalised zero, ``(0 - mean) / div``; frames past ``out_frames`` are cut."""
    B, n, nm = img.shape
    div = 1.0 if norm_div == 0 else float(np.float32(norm_div))
    out = np.full((B, out_frames, nm), (0.0 - float(np.float32(norm_mean))) / div, img.dtype)
    k = min(n, out_frames)
    out[:, :k] = img[:, :k]
    return out


def cut_patches(img, patch) -> np.ndarray:
    """``FbankPlan.patches``: ``[B, out_frames, n_mels]`` -> ``[B * nt * nf, patch * patch]`` with token = t * nf + f, the ragged edges dropped."""
    B, n, nm = img.shape
    nt, nf = n // patch, nm // patch
    return img[:, :nt * patch, :nf * patch].reshape(B, nt, patch, nf, patch).transpose(0, 1, 3, 2, 4).reshape(B * nt * nf, patch * patch)


# ------------------------------------------------------------------------------------------------------------------------
# STFT power / mel spectrogram (melspec.hip)
# ------------------------------------------------------------------------------------------------------------------------
def ramp_noise(B: int, T: int, seed: int) -> np.ndarray:
    """The STFT tests' input: N(0, 0.1^2) noise under an amplitude ramp from 1e-3 to 1 across the clip, so that every frame has its own level
    and a per-frame bar judges each at it (a quiet frame cannot hide behind a loud one)."""
    from avex_amd import synth
    return (synth.noise_clips(B, T, seed=seed) * np.linspace(1e-3, 1.0, T, dtype=np.float32)[None, :]).astype(np.float32)


def per_frame_excess(spec, ref, rel=3e-5) -> float:
    """max over (clip, frame) of  max_bins |spec - ref| / (rel * max_bins ref): <= 1 when every frame meets the per-frame bar."""
    err = np.abs(np.asarray(spec, np.float64) - ref).max(axis=1)
    return float((err / (rel * ref.max(axis=1))).max())


def stft_frames(T: int, n_fft: int, hop: int, center: bool) -> int:
    if center:
        return 1 + T // hop
    return 0 if T < n_fft else 1 + (T - n_fft) // hop


def stft_power64(wav, n_fft, hop, win_length, window, center) -> np.ndarray:
    """``|torch.stft|^2`` in fp64: ``[B, T]`` -> ``[B, n_fft // 2 + 1, frames]``.  ``center`` reflects ``n_fft // 2`` samples at each end
    (sample ``-j`` is sample ``j``); the window sits in the middle of the ``n_fft`` points, ``(n_fft - win_length) // 2`` zeros before it."""
    x = np.asarray(wav, np.float64)
    if center:
        x = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    w = np.zeros(n_fft)
    lo = (n_fft - win_length) // 2
    w[lo:lo + win_length] = np.asarray(window, np.float64)
    n = 1 + (x.shape[1] - n_fft) // hop
    fr = x[:, np.arange(n)[:, None] * hop + np.arange(n_fft)[None, :]] * w
    with np.errstate(invalid="ignore", over="ignore"):
        spec = np.fft.rfft(fr, axis=-1)
        return (spec.real ** 2 + spec.imag ** 2).transpose(0, 2, 1)


def melspec64(power, mel_fb=None, normalize=True) -> np.ndarray:
    """The rest of the reference's AudioProcessor: the ``[n_freq, n_mels]`` bank (or none), then ``log(x + 1e-6)`` and the per-clip
    ``(x - min) / (max - min + 1e-8)``.  The min and max PROPAGATE NaN (``Tensor.amin`` / ``amax`` do): one NaN makes the clip's image NaN."""
    x = np.asarray(power, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mel_fb is not None:
            x = np.einsum("fm,bft->bmt", np.asarray(mel_fb, np.float64), x)
        if normalize:
            x = np.log(x + MEL_LOG_EPS)
            mn = x.min(axis=(1, 2), keepdims=True)             # np.min / np.max propagate NaN
            mx = x.max(axis=(1, 2), keepdims=True)
            x = (x - mn) / (mx - mn + float(np.float32(1e-8)))
    return x


# ------------------------------------------------------------------------------------------------------------------------
# resamplers (ingest.hip)
# ------------------------------------------------------------------------------------------------------------------------
def sinc_plan(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(orig, new, width, taps) of the reduced ratio, as the kernel's plan holds them."""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    width = math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff))
    return orig, new, width, 2 * width + orig


def resample64(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, beta=0.0) -> np.ndarray:
    """torchaudio's windowed-sinc resampler, ``[B, T]`` -> ``[B, ceil(T * new / orig)]`` fp64: output ``q * new + p`` is the dot product of
    row ``p`` of the polyphase table (built in fp64, ROUNDED TO FP32 like the device's) with input samples ``q * orig - width ...``, zero
    outside the clip."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    orig, new, width, taps = sinc_plan(orig_freq, new_freq, lowpass_filter_width, rolloff)
    base = min(orig, new) * rolloff
    j = np.arange(taps, dtype=np.float64)
    p = np.arange(new, dtype=np.float64)
    t = ((j[None, :] - width) / orig - p[:, None] / new) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    if beta > 0:
        win = np.i0(beta * np.sqrt(1.0 - (t / lowpass_filter_width) ** 2)) / np.i0(beta)
    else:
        win = np.cos(t * math.pi / lowpass_filter_width / 2.0) ** 2
    a = t * math.pi
    table = (np.where(a == 0, 1.0, np.sin(a) / np.where(a == 0, 1.0, a)) * win * (base / orig)).astype(np.float32).astype(np.float64)
    B, T = x.shape
    n_out = -(-new * T // orig)
    nq = -(-n_out // new)
    xp = np.zeros((B, width + nq * orig + taps))
    xp[:, width:width + T] = x
    seg = xp[:, np.arange(nq)[:, None] * orig + np.arange(taps)[None, :]]           # [B, nq, taps]: samples q * orig - width + j
    return np.einsum("bqj,pj->bqp", seg, table).reshape(B, nq * new)[:, :n_out]


RESAMPY_KAISER_BEST = (64, 9, 0.9475937167399596, 14.769656459379492)      # zero crossings, table bits, rolloff, Kaiser beta (resampy's published filter)


def interp_wing(orig_sr, target_sr) -> int:
    """Input samples one wing of the interpolating filter reaches."""
    return math.ceil(RESAMPY_KAISER_BEST[0] / min(1.0, target_sr / orig_sr))


def resample_interp64(x, orig_sr, target_sr, scale=True) -> np.ndarray:
    """librosa.resample(res_type="kaiser_best") = resampy's interpolating resampler, ``[B, T]`` -> ``[B, ceil(T * ratio)]`` fp64: output ``t``
    sits at input time ``t / ratio``; each of its two wings walks the half-window table in steps of ``int(min(1, ratio) * 512)`` entries from
    the fractional offset, every weight interpolated linearly between neighbouring entries.  The table and its differences are ROUNDED TO
    FP32 like the device's; the interpolation and the sums are fp64.  ``int(T * ratio)`` samples are computed, the rest (at most one) is 0."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    nz, prec, rolloff, kbeta = RESAMPY_KAISER_BEST
    ratio = float(target_sr) / float(orig_sr)
    bits = 1 << prec
    n = bits * nz
    w = rolloff * np.sinc(rolloff * np.linspace(0, nz, num=n + 1, endpoint=True)) * np.kaiser(2 * n + 1, kbeta)[n:]
    sc = min(1.0, ratio)
    w = w * sc
    win = w.astype(np.float32).astype(np.float64)
    delta = np.zeros(n + 1)
    delta[:-1] = np.diff(w).astype(np.float32).astype(np.float64)
    step = int(sc * bits)
    B, T = x.shape
    n_res, n_out = int(T * ratio), int(math.ceil(T * ratio))
    out = np.zeros((B, n_out))
    for t in range(n_res):
        pos = t * (1.0 / ratio)
        i0 = int(pos)
        frac = sc * (pos - i0)
        acc = np.zeros(B)
        for wing in (0, 1):
            if wing:
                frac = sc - frac
            idx = frac * bits
            off = int(idx)
            eta = idx - off
            cnt = (n + 1 - off) // step
            cnt = min(cnt, i0 + 1) if wing == 0 else min(cnt, T - i0 - 1)
            if cnt <= 0:
                continue
            k = off + np.arange(cnt) * step
            src = (i0 - np.arange(cnt)) if wing == 0 else (i0 + 1 + np.arange(cnt))
            acc += x[:, src] @ (win[k] + eta * delta[k])
        out[:, t] = acc
    return out / math.sqrt(ratio) if scale else out


# ------------------------------------------------------------------------------------------------------------------------
# positional convolution (posconv.hip)
# ------------------------------------------------------------------------------------------------------------------------
def posconv64(xh, w, bias, groups, residual: Optional[np.ndarray] = None):
    """``residual + gelu(conv1d(xh))`` in fp64 on operands ALREADY ROUNDED to the half type: grouped Conv1d over time with kernel ``K = w.shape[2]``,
    padding ``K // 2`` and the last output dropped (even K), the erf GELU, then the residual (``xh`` itself when none is given).
    ``xh [B, T, E]``, ``w [E, E / groups, K]`` -> ``(out, conv)``, both ``[B, T, E]``; ``conv`` is the GELU output alone."""
    xh = np.asarray(xh, np.float64)
    w = np.asarray(w, np.float64)
    B, T, E = xh.shape
    K = w.shape[2]
    cg = E // groups
    pad = K // 2
    xp = np.pad(xh, ((0, 0), (pad, pad), (0, 0)))
    y = np.zeros((B, T, E))
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(groups):
            sl = slice(g * cg, (g + 1) * cg)
            xg = np.ascontiguousarray(xp[:, :, sl])
            wg = np.ascontiguousarray(w[sl].transpose(2, 1, 0))  # [K, c, o]
            acc = np.zeros((B, T, cg))
            for k in range(K):                                   # out[t] += x[t + k - pad] . w[:, :, k]
                acc += xg[:, k:k + T] @ wg[k]
            y[:, :, sl] = acc
        y = y + np.asarray(bias, np.float64)
        conv = 0.5 * y * (1.0 + _erf(y / math.sqrt(2.0)))
        return (xh if residual is None else np.asarray(residual, np.float64)) + conv, conv


def half_ulp(ref, dtype) -> np.ndarray:
    """Half a unit in the last place of the half type at ``|ref|`` (normal range): the distance rounding to that type may move a value."""
    mant = 10 if dtype in ("f16", 0) else 7
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(ref, np.float64)), 2.0 ** -14 if mant == 10 else 2.0 ** -126)))
    return 0.5 * 2.0 ** (e - mant)
