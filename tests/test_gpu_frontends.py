"""The audio front ends off their model settings: the kaldi filterbank (csrc/fbank.hip), the STFT / mel kernels (csrc/melspec.hip), the two
resamplers (csrc/ingest.hip) and the positional convolution (csrc/posconv.hip), each against the plain fp64 restatement of tests/_frontend_ref.py
(pinned to the oracles and to torch by tests/test_frontend_ref_cpu.py), at the smallest shapes that reach every branch: pad and cut rows, ragged
patches, row strides, frame counts around the frames per workgroup, clips barely longer than the reflect padding, every dense column tiling, clips
shorter than a filter wing, output lengths around a workgroup's 256 samples, token counts around the wave's 64 and the segment's 512, and NaN /
Inf containment.

Bars are the project's, applied locally:
    filterbank   tests/test_gpu_kernels.py::_fbank_close (2e-3 in energy with the 3e-6 * peak floor) and max |dlog| < 1e-3 on noise; half patches add
                 2^-11 (f16) / 2^-8 (bf16) of the reference value, half a unit of the output type
    STFT         max_bins |spec - ref| <= 3e-5 * max_bins ref for EACH (clip, frame); the normalised mel image 2e-4 absolute
    resamplers   2e-6 (windowed sinc) and 5e-6 (interpolating) absolute, input std 0.3
    posconv      the L2 error of each (clip, token) row over the RMS row norm of the reference of that clip < 2e-5
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _frontend_ref as F
from _util import round_half
from avex_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
F32_EPS = 1.1920929e-07
SENT = -1984.0          # exact in f16, bf16 and fp32


def _K():
    from avex_amd import kernels
    return kernels


def _err():
    from avex_amd._capi import AvexHipError
    return AvexHipError


def _tdt(name):
    return torch.float16 if name == "f16" else torch.bfloat16


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype)


def _np(t):
    return t.float().cpu().numpy() if t.dtype != torch.float32 else t.cpu().numpy()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


# ========================================================================================================================
# Filterbank
# ========================================================================================================================
class _Fb:
    """One filterbank setting: the device plan and the arguments of its fp64 reference."""

    def __init__(self, *, win=400, hop=160, preemph=0.97, remove_dc=True, input_scale=32768.0, n_mels=128, log_floor=F32_EPS, norm_mean=0.0,
                 norm_div=1.0, hann=False, low=20.0, high=0.0):
        K = _K()
        self.win, self.hop, self.n_mels, self.floor, self.mean, self.div = win, hop, n_mels, log_floor, norm_mean, norm_div
        window = K.hann_window(win) if hann else K.povey_window(win)
        mel_fb = K.kaldi_mel_filterbank(n_mels, low_freq=low, high_freq=high)
        self.ref_kw = dict(win=win, hop=hop, preemph=preemph, remove_dc=remove_dc, window=window, mel_fb=mel_fb, input_scale=input_scale)
        self.plan = K.FbankPlan(win_length=win, hop_length=hop, n_mels=n_mels, input_scale=input_scale, preemph=preemph, remove_dc=remove_dc,
                                log_floor=log_floor, norm_mean=norm_mean, norm_div=norm_div, window=window, mel_fb=mel_fb)

    def energy(self, x, clip_offset=None):
        return np.maximum(F.fbank64(x, clip_offset=clip_offset, **self.ref_kw), float(np.float32(self.floor)))

    def check(self, got, e, what):
        """got: device output [B, frames, n_mels] (normalised log); e: floored reference energies.  The project's two bars."""
        assert got.shape == e.shape, (what, got.shape, e.shape)
        if e.size == 0:
            return
        lg = got.astype(np.float64) * float(np.float32(self.div)) + float(np.float32(self.mean))
        dlog = float(np.abs(lg - np.log(e)).max())
        peak = e.max(axis=-1, keepdims=True)
        eerr = float((np.abs(np.exp(lg) - e) / (e + 3e-6 * peak)).max())
        print(f"{what}: max |dlog| {dlog:.3e}, energy-domain {eerr:.3e}")
        assert eerr < 2e-3, what
        assert dlog < 1e-3, what


FB_GRID = [
    dict(win=64, hop=80, preemph=0.0, remove_dc=False, input_scale=1.0, n_mels=40),
    dict(win=64, hop=160, preemph=0.97, remove_dc=True, input_scale=32768.0, n_mels=80, hann=True),
    dict(win=200, hop=80, preemph=0.97, remove_dc=False, input_scale=32768.0, n_mels=128, log_floor=1.0, norm_mean=3.5, norm_div=2.5),
    dict(win=200, hop=400, preemph=0.0, remove_dc=True, input_scale=1.0, n_mels=40, low=100.0, high=-500.0),
    dict(win=400, hop=640, preemph=0.97, remove_dc=True, input_scale=1.0, n_mels=80, log_floor=1e-4, norm_mean=-4.268, norm_div=9.138, hann=True),
    dict(win=400, hop=160, preemph=0.0, remove_dc=False, input_scale=32768.0, n_mels=128),
    dict(win=400, hop=400, preemph=0.97, remove_dc=False, input_scale=1.0, n_mels=40, norm_mean=1.25, norm_div=0.5),
    dict(win=512, hop=80, preemph=0.97, remove_dc=True, input_scale=32768.0, n_mels=80),
    dict(win=512, hop=640, preemph=0.0, remove_dc=False, input_scale=1.0, n_mels=128, norm_mean=15.41663, norm_div=13.11164, hann=True),
    dict(win=512, hop=160, preemph=0.0, remove_dc=True, input_scale=32768.0, n_mels=40, low=0.0, high=4000.0),
    dict(win=64, hop=640, preemph=0.97, remove_dc=False, input_scale=32768.0, n_mels=128, log_floor=1e3),
    dict(win=200, hop=160, preemph=0.97, remove_dc=True, input_scale=1.0, n_mels=80, norm_mean=-2.0, norm_div=3.0),
]


@pytest.mark.parametrize("i", range(len(FB_GRID)))
def test_fbank_settings_grid(built_lib, i):
    """Window lengths that leave whole lane steps empty (64, 200), hop >= win, no pre-emphasis, no DC removal, both input scales, other floors and
    affines, 40 / 80 / 128 mels with their own banks and windows, on [3, 4000] noise."""
    fb = _Fb(**FB_GRID[i])
    x = synth.noise_clips(3, 4000, seed=100 + i)
    got = fb.plan(_dev(x)).cpu().numpy()
    assert got.shape == (3, F.fbank_frames(4000, fb.win, fb.hop), fb.n_mels)
    fb.check(got, fb.energy(x), f"grid {FB_GRID[i]}")


@pytest.mark.parametrize("win,hop", [(400, 160), (200, 240)])
def test_fbank_frame_counts_around_the_workgroup(built_lib, win, hop):
    """1, 2, 7, 8, 9, 15, 16, 17 frames (a workgroup holds 8: four waves of one frame pair), at the shortest clip with that many and at the
    longest, three clips per call."""
    fb = _Fb(win=win, hop=hop, n_mels=40, input_scale=1.0)
    for n in (1, 2, 7, 8, 9, 15, 16, 17):
        for T in (win + (n - 1) * hop, win + (n - 1) * hop + hop - 1):
            x = synth.noise_clips(3, T, seed=200 + n)
            got = fb.plan(_dev(x)).cpu().numpy()
            assert got.shape == (3, n, 40)
            fb.check(got, fb.energy(x), f"{n} frames, T={T}")


@pytest.mark.parametrize("clip_mean", [False, True])
def test_fbank_padded_rows(built_lib, clip_mean):
    """out_frames below, at and above the frame count (odd and even): rows past the last frame hold (0 - mean) / div exactly, the rows below are
    the bits of the call without padding, and agree with the fp64 reference."""
    fb = _Fb(n_mels=80, input_scale=1.0, remove_dc=not clip_mean, norm_mean=-4.268, norm_div=9.138, hann=True)
    x = synth.noise_clips(3, 4000, seed=210) + np.float32(0.05)
    xd = _dev(x)
    frames = fb.plan.num_frames(4000)
    assert frames == 23
    base = fb.plan.padded(xd, frames, remove_clip_mean=True) if clip_mean else fb.plan(xd)
    e = fb.energy(x, clip_offset=x.astype(np.float64).mean(axis=1) if clip_mean else None)
    fb.check(base.cpu().numpy(), e, f"padded base clip_mean={clip_mean}")
    pad_value = (np.float32(0.0) - np.float32(fb.mean)) / np.float32(fb.div)
    for out_frames in (frames - 3, frames, frames + 1, frames + 9):
        got = fb.plan.padded(xd, out_frames, remove_clip_mean=clip_mean)
        assert got.shape == (3, out_frames, 80)
        k = min(frames, out_frames)
        assert np.array_equal(_bits(got[:, :k]), _bits(base[:, :k])), out_frames
        assert (got[:, k:].cpu().numpy() == pad_value).all(), out_frames


def _patches_guarded(fb, xd, out_frames, patch, dtype, clip_mean=False):
    """FbankPlan.patches through the C entry point into a buffer with sentinel rows behind the last token."""
    from avex_amd._capi import check, dtype_code, lib
    B, T = xd.shape
    n = out_frames if out_frames > 0 else fb.plan.num_frames(T)
    rows = B * (n // patch) * (fb.n_mels // patch)
    buf = torch.full((rows + 16, patch * patch), SENT, dtype=_tdt(dtype), device="cuda")
    off = None
    if clip_mean:
        off = torch.empty((B,), dtype=torch.float32, device="cuda")
        check(lib().avexhip_clip_mean(xd.data_ptr(), B, T, xd.stride(0), off.data_ptr(), _stream()), "clip_mean")
    check(lib().avexhip_fbank_forward_patches(fb.plan._h, xd.data_ptr(), B, T, xd.stride(0), off.data_ptr() if off is not None else None, out_frames, patch,
                                              buf.data_ptr(), dtype_code(dtype), _stream()), "fbank_forward_patches")
    assert (buf[rows:].float() == SENT).all(), "the patch kernel wrote behind the last token"
    return buf[:rows]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("patch,n_mels,out_frames", [(8, 40, 23), (8, 128, 30), (16, 80, 37), (16, 128, 20), (32, 80, 37), (32, 128, 64), (16, 80, 0)])
def test_fbank_patches(built_lib, dtype, patch, n_mels, out_frames):
    """Patch sizes 8 / 16 / 32 in both half types with ragged edges: out_frames no multiple of the patch (23, 30, 37, 20), mel counts no multiple
    (40 % 16, 80 % 32), out_frames above the 23 frames (pad rows inside patches) and below.  The values are the fp32 padded output of the same
    call rounded to the type and cut into patches, bit for bit; nothing is written behind the last token; and the fp64 reference holds."""
    fb = _Fb(n_mels=n_mels, input_scale=1.0, norm_mean=-4.268, norm_div=9.138)
    x = synth.noise_clips(3, 4000, seed=220)
    xd = _dev(x)
    n = out_frames if out_frames > 0 else 23
    got = _patches_guarded(fb, xd, out_frames, patch, dtype)
    assert got.shape == (3 * (n // patch) * (n_mels // patch), patch * patch)
    img = fb.plan.padded(xd, n)
    want = F.cut_patches(img.to(_tdt(dtype)).cpu().view(torch.int16).numpy(), patch)
    assert np.array_equal(_bits(got), want)
    # the wrapper gives the same rows
    assert np.array_equal(_bits(fb.plan.patches(xd, out_frames, patch, dtype=dtype)), _bits(got))
    ref = F.cut_patches(F.fbank_pad(F.fbank_log(fb.energy(x), fb.floor, fb.mean, fb.div), n, fb.mean, fb.div), patch)
    bar = 1e-3 / float(np.float32(fb.div)) + np.abs(ref) * (2.0 ** -11 if dtype == "f16" else 2.0 ** -8)
    excess = float((np.abs(_np(got).astype(np.float64) - ref) / bar).max())
    print(f"patches {patch} {n_mels} {out_frames} {dtype}: {excess:.3f} of the bar")
    assert excess <= 1.0


def test_fbank_patches_with_the_clip_mean(built_lib):
    fb = _Fb(n_mels=128, input_scale=1.0, remove_dc=False, hann=True)
    xd = _dev(synth.noise_clips(3, 4000, seed=221) + np.float32(0.05))
    got = _patches_guarded(fb, xd, 32, 16, "f16", clip_mean=True)
    want = F.cut_patches(fb.plan.padded(xd, 32, remove_clip_mean=True).half().cpu().view(torch.int16).numpy(), 16)
    assert np.array_equal(_bits(got), want)


def test_fbank_row_stride(built_lib):
    """A [3, T] view of a [3, T + 77] buffer whose tail holds 1e30: the bits of the contiguous copy, in all three outputs."""
    fb = _Fb(n_mels=80, input_scale=1.0)
    T = 4000
    wide = torch.full((3, T + 77), 1e30, dtype=torch.float32, device="cuda")
    wide[:, :T] = _dev(synth.noise_clips(3, T, seed=230))
    view = wide[:, :T]
    tight = view.contiguous()
    assert view.stride(0) == T + 77 and tight.stride(0) == T
    assert np.array_equal(_bits(fb.plan(view)), _bits(fb.plan(tight)))
    assert np.array_equal(_bits(fb.plan.padded(view, 30, remove_clip_mean=True)), _bits(fb.plan.padded(tight, 30, remove_clip_mean=True)))
    assert np.array_equal(_bits(fb.plan.patches(view, 32, 16)), _bits(fb.plan.patches(tight, 32, 16)))
    assert bool(torch.isfinite(fb.plan(view)).all())


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("s", [0, 1234, 1439, 3999])
def test_fbank_nan_stays_in_its_frames(built_lib, value, s):
    """One NaN (or Inf: the per-frame mean makes it NaN) sample in clip 1 of 3: every frame whose window holds it is NaN in every bin, the other
    clips have the bits of the clean run, and inside the poisoned clip nothing else is non-finite except the frame that shares the FFT of such a
    frame.  KNOWN DEVIATION: frames 2k and 2k + 1 are packed as one complex sequence, so a NaN in one reaches its partner; the
    reference transforms every frame alone and keeps the partner finite."""
    fb = _Fb()
    x = synth.noise_clips(3, 4000, seed=240)
    clean = fb.plan(_dev(x))
    bad = x.copy()
    bad[1, s] = value
    got = fb.plan(_dev(bad))
    for b in (0, 2):
        assert np.array_equal(_bits(got[b]), _bits(clean[b]))
    g = got[1].cpu().numpy()
    frames = g.shape[0]
    holds = np.array([f * 160 <= s < f * 160 + 400 for f in range(frames)])
    partner = holds[np.minimum(np.arange(frames) ^ 1, frames - 1)] & ~holds          # frames 2k and 2k + 1 share a transform
    assert np.isnan(g[holds]).all()
    rest = ~(holds | partner)
    assert np.array_equal(_bits(got[1])[rest], _bits(clean[1])[rest])
    assert np.isfinite(g[rest]).all()
    ref = F.fbank64(bad, **fb.ref_kw)
    assert np.array_equal(np.isnan(ref[1]).all(axis=-1), holds) and np.array_equal(np.isnan(ref[1]).any(axis=-1), holds)


# ========================================================================================================================
# STFT / mel
# ========================================================================================================================
def _stft_fb(n_fft, n_out, dense=False):
    """Frames per workgroup of the kernel a plan takes (melspec.hip: the dense product always 32; the FFT kernel 32 when the twiddles, four waves'
    ping-pong buffers and the [n_out][33] staging tile fit 160 KB of LDS, else 16)."""
    if dense:
        return 32
    return 32 if 8 * (n_fft + 4 * 2 * n_fft) + 4 * n_out * 33 <= 160 * 1024 else 16


def _stft_check(n_fft, hop, T, *, win=None, window="hann", center=True, n_mels=0, seed=300, what=""):
    """Plain power spectrum per frame, and (n_mels > 0) the normalised mel image, of [3, T] ramped noise."""
    K = _K()
    win = win or n_fft
    x = F.ramp_noise(3, T, seed)
    xd = _dev(x)
    w = K.stft_window(window, win)
    ref = F.stft_power64(x, n_fft, hop, win, w, center)
    spec = K.MelspecPlan(n_fft=n_fft, hop_length=hop, win_length=win, window=window, mel=False, center=center, normalize=False)(xd).cpu().numpy()
    assert spec.shape == ref.shape == (3, n_fft // 2 + 1, F.stft_frames(T, n_fft, hop, center)), what
    ex = F.per_frame_excess(spec, ref)
    line = f"stft {what} n_fft={n_fft} hop={hop} T={T} frames={ref.shape[2]}: {ex:.3f} of the per-frame bar"
    if n_mels:
        y = K.MelspecPlan(n_fft=n_fft, hop_length=hop, win_length=win, window=window, n_mels=n_mels, center=center, normalize=True)(xd).cpu().numpy()
        yr = F.melspec64(ref, K.htk_mel_filterbank(n_fft // 2 + 1, n_mels, 16000))
        assert y.shape == yr.shape
        d = float(np.abs(y - yr).max())
        line += f", mel image {d:.2e}"
        print(line)
        assert d < 2e-4, line
    else:
        print(line)
    assert ex <= 1.0, line


@pytest.mark.parametrize("n_fft,n_mels", [(96, 16), (400, 40), (800, 128), (2048, 64)])
def test_stft_short_clips_and_frame_counts(built_lib, n_fft, n_mels):
    """Clips of n_fft // 2 + 1 samples (the two reflect pads meet: every sample but one is read twice) and n_fft; 1, 2, 3 frames (hop = n_fft);
    FB - 1, FB, FB + 1 and 2 FB + 1 frames for both workgroup sizes the FFT kernel takes (16: the 2048-point power spectrum; 32: the rest)."""
    hs = n_fft // 4
    counts = sorted({n for fb in (_stft_fb(n_fft, n_fft // 2 + 1), _stft_fb(n_fft, n_mels)) for n in (fb - 1, fb, fb + 1, 2 * fb + 1)})
    assert _stft_fb(2048, 1025) == 16 and _stft_fb(2048, 64) == 32 and _stft_fb(800, 401) == 32
    for T in (n_fft // 2 + 1, n_fft):
        _stft_check(n_fft, hs, T, n_mels=n_mels, what="short")
    for T in (n_fft // 2 + 1, n_fft + 5, 2 * n_fft + 5):                  # 1, 2, 3 frames
        _stft_check(n_fft, n_fft, T, n_mels=n_mels, what="few")
    for n in counts:
        _stft_check(n_fft, hs, (n - 1) * hs + 3, n_mels=n_mels, what=f"{n} frames")


def test_stft_uncentred_gapped_and_short_window(built_lib):
    _stft_check(512, 128, 512, center=False, n_mels=64, what="uncentred, one frame")
    _stft_check(512, 128, 512 + 127, center=False, n_mels=64, what="uncentred, still one frame")
    _stft_check(512, 128, 512 + 128 * 32, center=False, n_mels=64, what="uncentred, 33 frames")
    _stft_check(400, 440, 3000, n_mels=40, what="hop = n_fft + 40")
    _stft_check(308, 348, 3000, n_mels=40, what="dense, hop = n_fft + 40")
    _stft_check(400, 100, 3000, win=301, window="hamming", n_mels=40, what="win 301 of 400")
    _stft_check(400, 100, 3000, win=301, window="hann", n_mels=40, what="hann 301 of 400")
    _stft_check(308, 77, 3000, win=201, window="hamming", n_mels=40, what="dense, win 201 of 308 (window not symmetric about n_fft / 2)")
    _stft_check(308, 77, 3000, win=201, window="hann", n_mels=40, what="dense, hann 201 of 308")


@pytest.mark.parametrize("n_fft,tiling", [(308, 3), (462, 4), (574, 5), (770, 7), (1024, 9)])
def test_stft_dense_column_tilings(built_lib, monkeypatch, n_fft, tiling):
    """The dense fp32-MFMA product with every instantiated column tiling (lengths with a prime factor above 5; 1024 forced onto it)."""
    assert ((n_fft // 2 + 1 + 63) // 64) == tiling
    monkeypatch.setenv("AVEX_AMD_MELSPEC_DENSE", "1")
    hs = n_fft // 4
    for T in (n_fft // 2 + 1, 30 * hs + 3, 32 * hs + 3, 64 * hs + 3):     # short; 31, 33 and 65 frames
        _stft_check(n_fft, hs, T, n_mels=40, what=f"dense tiling {tiling}")
    _stft_check(n_fft, n_fft // 2 + 2, n_fft // 2 + 1, n_mels=40, what=f"dense tiling {tiling}, one frame")


def test_stft_refusals(built_lib):
    K = _K()
    E = _err()
    for n_fft in (686, 1022):                                             # column tilings 6 and 8: not instantiated
        with pytest.raises(E, match=r"dense path: n_fft 256\.\.382, 384\.\.510, 512\.\.638, 768\.\.894, 1024\)"):
            K.MelspecPlan(n_fft=n_fft, hop_length=160, mel=False, normalize=False)
    for kw in (dict(n_fft=401, hop_length=100), dict(n_fft=62, hop_length=16), dict(n_fft=400, hop_length=100, win_length=401)):
        with pytest.raises(E):
            K.MelspecPlan(mel=False, normalize=False, **kw)
    plan = K.MelspecPlan(n_fft=400, hop_length=100, mel=False, normalize=False)
    with pytest.raises(E, match="reflect padding"):
        plan(_dev(F.ramp_noise(2, 200, 1)))
    assert plan(_dev(F.ramp_noise(2, 201, 1))).shape == (2, 201, 3)


@pytest.mark.parametrize("n_fft", [400, 308])
def test_mel_minmax(built_lib, n_fft):
    """A clip whose log values are all negative (the ordered-integer keys of negative floats), one that straddles zero, and an all-zero clip:
    min = max there and the image is 0 everywhere."""
    K = _K()
    T = 3000
    x = np.stack([synth.noise_clips(1, T, seed=310, amp=1e-3)[0], F.ramp_noise(1, T, 311)[0], np.zeros(T, np.float32)])
    plan = K.MelspecPlan(n_fft=n_fft, hop_length=100, n_mels=40, normalize=True)
    y = plan(_dev(x)).cpu().numpy()
    p = F.stft_power64(x, n_fft, 100, n_fft, K.stft_window("hann", n_fft), True)
    fbm = K.htk_mel_filterbank(n_fft // 2 + 1, 40, 16000)
    logs = np.log(np.einsum("fm,bft->bmt", fbm.astype(np.float64), p) + F.MEL_LOG_EPS)
    assert logs[0].max() < 0 and logs[1].min() < 0 < logs[1].max()
    ref = F.melspec64(p, fbm)
    assert float(np.abs(y - ref).max()) < 2e-4
    assert (y[2] == 0).all()
    for b in (0, 1):
        assert y[b].min() == 0.0 and abs(float(y[b].max()) - 1.0) < 1e-6


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("n_fft", [400, 308])
def test_mel_nan_poisons_its_clip_and_only_it(built_lib, n_fft, value):
    """One NaN or Inf sample in clip 1 of 3.  Normalised: the whole image of clip 1 is NaN, as the reference's amin / amax make it (the kernel's
    fminf / fmaxf used to skip the NaN and normalise the rest of the clip by a min and max that ignored it); clips 0 and 2 keep the bits of the
    clean run.  Not normalised: the frames that hold the sample are not finite, and only they and (FFT kernel, n_fft 400) the frame packed into
    the same complex transform."""
    K = _K()
    T, hop, s = 4000, 100, 2222
    x = F.ramp_noise(3, T, 320)
    bad = x.copy()
    bad[1, s] = value
    w = K.stft_window("hann", n_fft)
    fbm = K.htk_mel_filterbank(n_fft // 2 + 1, 40, 16000)
    plan = K.MelspecPlan(n_fft=n_fft, hop_length=hop, n_mels=40, normalize=True)
    clean, got = plan(_dev(x)), plan(_dev(bad))
    ref = F.melspec64(F.stft_power64(bad, n_fft, hop, n_fft, w, True), fbm)
    assert np.isnan(ref[1]).all()
    assert bool(torch.isnan(got[1]).all())
    for b in (0, 2):
        assert np.array_equal(_bits(got[b]), _bits(clean[b]))
        assert float(np.abs(got[b].cpu().numpy() - ref[b]).max()) < 2e-4
    for mel in (False, True):
        rplan = K.MelspecPlan(n_fft=n_fft, hop_length=hop, n_mels=40, mel=mel, normalize=False)
        rc, rg = rplan(_dev(x)), rplan(_dev(bad))
        frames = rg.shape[2]
        holds = np.array([f * hop - n_fft // 2 <= s < f * hop + n_fft - n_fft // 2 for f in range(frames)])
        pr = np.minimum(np.arange(frames) ^ 1, frames - 1)
        rest = ~(holds | holds[pr])
        g = rg[1].cpu().numpy()
        if math.isnan(value):
            assert np.isnan(g[:, holds]).all()
        else:
            assert not np.isfinite(g[:, holds]).any()
        assert np.array_equal(_bits(rg[1])[:, rest], _bits(rc[1])[:, rest])
        if n_fft == 308:                                                   # the dense product transforms every frame alone
            assert np.array_equal(_bits(rg[1])[:, ~holds], _bits(rc[1])[:, ~holds])
        for b in (0, 2):
            assert np.array_equal(_bits(rg[b]), _bits(rc[b]))


# ========================================================================================================================
# Resamplers
# ========================================================================================================================
RATIOS = [(48000, 8000), (16000, 48000), (44100, 48000), (11025, 16000), (44100, 16000)]


def _out_len(orig, new, T, interp):
    return int(math.ceil(T * (float(new) / float(orig)))) if interp else -(-(new // math.gcd(orig, new)) * T // (orig // math.gcd(orig, new)))


def _lengths(orig, new, interp):
    """1, 2, 5, one below and one above the filter's reach, and the shortest clips whose output has at least 255, 256, 257 and 513 samples
    (exactly those where the ratio can produce them: 16 000 -> 48 000 only makes multiples of 3)."""
    w = F.interp_wing(orig, new) if interp else F.sinc_plan(orig, new)[2]
    Ts = [1, 2, 5, w - 1, w + 1]
    for n in (255, 256, 257, 513):
        T = max(1, int(n * orig / new) - 2)
        while _out_len(orig, new, T, interp) < n:
            T += 1
        Ts.append(T)
    return sorted(set(t for t in Ts if t >= 1))


@pytest.mark.parametrize("interp", [False, True])
@pytest.mark.parametrize("orig,new", RATIOS)
def test_resamplers_short_clips_and_block_edges(built_lib, orig, new, interp):
    """Reduced new rate 1 (48 000 -> 8 000), above a workgroup's 256 outputs (11 025 -> 16 000: 640), 147 -> 160, up by 3; clips shorter than the
    filter's reach (the interpolating resampler's n + 1 and T - n - 1 clamps at T = 1) and outputs of 255, 256, 257 and 513 samples."""
    from avex_amd.ingest import Resampler
    rs = Resampler(orig, new, res_type="kaiser_best" if interp else None)
    bar = 5e-6 if interp else 2e-6
    rng = np.random.default_rng(orig + 7 * new + interp)
    lens = _lengths(orig, new, interp)
    outs = set()
    worst = 0.0
    for T in lens:
        x = (rng.standard_normal((3, T)) * 0.3).astype(np.float32)
        got = rs(_dev(x)).cpu().numpy()
        ref = F.resample_interp64(x, orig, new) if interp else F.resample64(x, orig, new)
        assert got.shape == ref.shape == (3, _out_len(orig, new, T, interp)), T
        outs.add(got.shape[1])
        worst = max(worst, float(np.abs(got - ref).max()))
        assert float(np.abs(got - ref).max()) < bar, (T, got.shape)
    print(f"resample {orig}->{new} interp={interp}: lengths {lens} -> worst {worst:.2e}")
    if new < orig:
        assert {255, 256, 257, 513} <= outs


@pytest.mark.parametrize("interp", [False, True])
def test_resamplers_row_strides(built_lib, interp):
    """Through the C entry point with x_stride = T + 13 and out_stride = n_out + 7: the guard columns keep their sentinel, the gaps of the input
    (1e30) are never read into a result, and a clip run alone gives the bits it has in the batch."""
    from avex_amd._capi import check, lib
    from avex_amd.ingest import Resampler
    orig, new, T = 44100, 16000, 1500
    rs = Resampler(orig, new, res_type="kaiser_best" if interp else None)
    n_out = rs.out_length(T)
    x = (np.random.default_rng(9).standard_normal((3, T)) * 0.3).astype(np.float32)
    xw = torch.full((3, T + 13), 1e30, dtype=torch.float32, device="cuda")
    xw[:, :T] = _dev(x)
    out = torch.full((3, n_out + 7), SENT, dtype=torch.float32, device="cuda")
    check(lib().avexhip_resample_forward(rs._h, xw.data_ptr(), 3, T, T + 13, out.data_ptr(), n_out + 7, _stream()), "resample_forward")
    assert (out[:, n_out:] == SENT).all()
    tight = rs(_dev(x))
    assert np.array_equal(_bits(out[:, :n_out]), _bits(tight))
    for b in range(3):
        assert np.array_equal(_bits(rs(_dev(x[b]))), _bits(tight[b]))
    ref = F.resample_interp64(x, orig, new) if interp else F.resample64(x, orig, new)
    assert float(np.abs(tight.cpu().numpy() - ref).max()) < (5e-6 if interp else 2e-6)


def test_resampler_refusals(built_lib):
    from avex_amd._capi import check, lib
    from avex_amd.ingest import Resampler
    E = _err()
    with pytest.raises(E, match="table or staging too large"):
        Resampler(16000, 15999)
    with pytest.raises(E, match="ratio too small"):
        Resampler(48000, 50, res_type="kaiser_best")                      # index_step = int(50 / 48000 * 512) = 0
    for interp in (False, True):
        rs = Resampler(32000, 16000, res_type="kaiser_best" if interp else None)
        x = torch.zeros((2, 100), dtype=torch.float32, device="cuda")
        out = torch.full((2, 64), SENT, dtype=torch.float32, device="cuda")
        with pytest.raises(E, match="x_stride"):                          # x_stride < T with B > 1: rows would overlap
            check(lib().avexhip_resample_forward(rs._h, x.data_ptr(), 2, 100, 99, out.data_ptr(), 50, _stream()), "resample_forward")
        with pytest.raises(E, match="out_stride"):                        # out_stride < n_out
            check(lib().avexhip_resample_forward(rs._h, x.data_ptr(), 2, 100, 100, out.data_ptr(), 49, _stream()), "resample_forward")
        torch.cuda.synchronize()
        assert (out == SENT).all()                                        # nothing was launched
        assert lib().avexhip_resample_forward(rs._h, x.data_ptr(), 2, 100, 100, out.data_ptr(), 50, _stream()) == 0
        assert (out.reshape(-1)[:100] == 0).all() and (out.reshape(-1)[100:] == SENT).all()


# ========================================================================================================================
# Positional convolution
# ========================================================================================================================
CG, KT = 48, 128
_PC = {}


def _pc_weights(G, dtype):
    """Packed weights of a G-group convolution (once per shape and type), the unpacked rounded weights [E, 48, 128] the reference uses, the bias."""
    key = (G, dtype)
    if key not in _PC:
        K = _K()
        E = CG * G
        v = synth.normal(f"fpcv{G}", (E, CG, KT), math.sqrt(1.0 / (KT * CG)))
        g = (np.sqrt((v.astype(np.float64) ** 2).sum((0, 1), keepdims=True)) * (1.0 + synth.normal(f"fpcg{G}", (1, 1, KT), 0.1))).astype(np.float32)
        bias = synth.normal(f"fpcb{G}", (E,), 0.05)
        wp = K.posconv_pack(_dev(g), _dev(v), G, dtype)
        # packed layout [g][u][v][g4][o][8], k = tap * 48 + c = 96 u + 32 v + 8 g4 + e  ->  [E][c][tap]
        wq = wp.float().cpu().numpy().reshape(G, KT * CG // 96, 3, 4, CG, 8).transpose(0, 4, 1, 2, 3, 5).reshape(G, CG, KT, CG)
        wq = np.ascontiguousarray(wq.transpose(0, 1, 3, 2).reshape(E, CG, KT))
        w_true = v.astype(np.float64) * (g.astype(np.float64) / np.sqrt((v.astype(np.float64) ** 2).sum((0, 1), keepdims=True)))
        assert np.abs(wq - w_true).max() <= np.abs(w_true).max() * (2.0 ** -10 if dtype == "f16" else 2.0 ** -7)
        _PC[key] = (wp, wq, bias)
    return _PC[key]


def _row_excess(got, ref, conv):
    """max over rows of  ||got - ref||_2 / (2e-5 * rms_t ||conv||_2 of the clip)."""
    err = np.linalg.norm(got.astype(np.float64) - ref, axis=-1)
    rms = np.sqrt((np.linalg.norm(conv, axis=-1) ** 2).mean(axis=1, keepdims=True))
    return float((err / (2e-5 * rms)).max())


def _pc_case(G, T, dtype, B=3):
    K = _K()
    E = CG * G
    wp, wq, bias = _pc_weights(G, dtype)
    x = synth.normal(f"fpcx{G}_{T}", (B, T, E), 1.0)
    xh = round_half(x, dtype)
    refh, conv = F.posconv64(xh, wq, bias, G)                 # the half residual; the fp32 one differs by the residual alone
    ref = x.astype(np.float64) + conv
    out = K.posconv(_dev(xh, _tdt(dtype)), _dev(x), wp, _dev(bias), G, KT)
    assert out.dtype == torch.float32 and out.shape == (B, T, E)
    ex = _row_excess(out.cpu().numpy(), ref, conv)
    # operand-type residual and output
    outh =K.posconv(_dev(xh, _tdt(dtype)), None, wp, _dev(bias), G, KT, half_out=True)
    assert outh.dtype == _tdt(dtype) and outh.shape == (B, T, E)
    rms_el = np.sqrt((conv ** 2).mean())
    slack = np.abs(_np(outh).astype(np.float64) - refh) - F.half_ulp(refh, dtype)
    print(f"posconv G={G} T={T} {dtype}: {ex:.3f} of the per-row bar; half output beyond half an ulp by {slack.max():.2e}")
    assert ex <= 1.0
    exact = np.array_equal(_np(outh), round_half(refh.astype(np.float32), dtype))
    assert exact or slack.max() <= 2e-5 * rms_el


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 63, 64, 65, 511, 512, 513, 1024, 1025])
@pytest.mark.parametrize("G", [1, 3])
def test_posconv_token_counts(built_lib, G, T, dtype):
    """One and three groups of 48 channels (all the kernel's shape depends on) at the wave's 64 tokens, the 64-row halo and the 512-token
    segment ends, each (clip, token) row judged on its own."""
    _pc_case(G, T, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_posconv_model_width(built_lib, dtype):
    _pc_case(16, 65, dtype, B=2)


def test_posconv_saturates_f16(built_lib):
    """Inputs of magnitude 6e4 with the f16 output: sums past the type's range come out as a finite +-65504, not inf."""
    K = _K()
    G, T = 1, 70
    wp, wq, bias = _pc_weights(G, "f16")
    sign = np.where(synth.normal("fpcsat", (2, T, CG), 1.0) >= 0, 1.0, -1.0).astype(np.float32)
    xh = round_half(sign * np.float32(6e4), "f16")
    out = _np(K.posconv(_dev(xh, torch.float16), None, wp, _dev(bias), G, KT, half_out=True))
    ref, _ = F.posconv64(xh, wq, bias, G)
    assert np.isfinite(out).all()
    over = ref > 65520.0
    assert over.sum() > 100
    assert (out[over] == 65504.0).all()
    assert np.abs(out).max() == 65504.0
    inside = np.abs(ref) < 65000.0
    assert np.abs(out[inside] - ref[inside]).max() <= 16.0 + 0.5          # half a unit of f16 at 2^15..2^16, and the fp32 sum's own error


@pytest.mark.parametrize("T,t", [(130, 0), (130, 129), (1025, 511), (1025, 512), (1025, 1024)])
def test_posconv_nan_stays_in_its_taps(built_lib, T, t):
    """A NaN at (clip 1, token t, one channel of group 1): group 1 of clip 1 is NaN at tokens t - 63 .. t + 64, the taps that read it, and nowhere
    else; the other groups and clips have the bits of the clean run.  t = 511 / 512 at T = 1025 crosses a segment's halo."""
    K = _K()
    G, E = 3, 3 * CG
    wp, wq, bias = _pc_weights(G, "f16")
    x = synth.normal(f"fpcn{T}", (3, T, E), 1.0)
    xh = round_half(x, "f16")
    bad = xh.copy()
    bad[1, t, CG + 5] = np.nan
    for half_out in (False, True):
        run = lambda a: K.posconv(_dev(a, torch.float16), None if half_out else _dev(x), wp, _dev(bias), G, KT, half_out=half_out)
        clean, got = run(xh), run(bad)
        nan = torch.isnan(got).cpu().numpy()
        want = np.zeros((3, T, E), bool)
        want[1, max(0, t - 63):min(T, t + 65), CG:2 * CG] = True
        assert np.array_equal(nan, want)
        assert np.array_equal(_bits(got)[~want], _bits(clean)[~want])
        assert bool(torch.isfinite(clean).all())


def test_posconv_pack_refuses_shapes_its_layout_cannot_hold(built_lib):
    """The packed layout is whole 96-wide tap pairs per group: E = 64, two groups, K = 128 (32 * 128 % 96 != 0) made the blocks overlap and, with one
    group, run past the buffer.  48 channels per group still pack."""
    K = _K()
    v = _dev(synth.normal("fpcbadv", (64, 32, 128), 0.1))
    g = _dev(np.ones((1, 1, 128), np.float32))
    with pytest.raises((ValueError, _err()), match="multiple of 96"):
        K.posconv_pack(g, v, 2, "f16")
    with pytest.raises((ValueError, _err())):
        K.posconv_pack(_dev(np.ones((1, 1, 100), np.float32)), _dev(synth.normal("fpcbadv2", (40, 40, 100), 0.1)), 1, "bf16")
    wp, wq, _ = _pc_weights(1, "bf16")
    assert wp.numel() == CG * CG * KT and np.isfinite(wq).all()
