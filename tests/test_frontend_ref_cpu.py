"""Pins tests/_frontend_ref.py (the fp64 restatements tests/test_gpu_frontends.py judges the front-end kernels by) against what the project
already trusts: the fp32 oracles under oracle/ and torch itself.  No GPU.

Measured gaps, fp32 oracle against the fp64 restatement (asserted at four times these, so the restatement cannot drift):
    fbank, synth.noise_clips(2, 16000, seed=0), input scale 2**15 and 1.0     max |log difference|                 7.6e-5
    the same                                                                   energy-domain error, _fbank_close   9e-6
    fbank, synth.tone_clips(16000) * 2**15                                     energy-domain error, _fbank_close   1.8e-5
so the project's bars (1e-3 in log, 2e-3 in energy with the 3e-6 * peak floor) hold against the fp64 reference with about 100x to spare."""
import math

import numpy as np
import pytest
import torch

import _frontend_ref as F
from avex_amd import synth
from oracle import beats_oracle as O
from oracle import ingest_oracle as IO

FBANK_LOG_GAP, FBANK_ENERGY_GAP, FBANK_TONE_GAP = 7.6e-5, 9e-6, 1.8e-5


def _energy_err(log_a, e_ref):
    """tests/test_gpu_kernels.py::_fbank_close's measure, the reference given as energies."""
    ea = np.exp(np.asarray(log_a, np.float64))
    peak = e_ref.max(axis=-1, keepdims=True)
    return float((np.abs(ea - e_ref) / (e_ref + 3e-6 * peak)).max())


def _fbank64_default(x, scale):
    return np.maximum(F.fbank64(x, win=400, hop=160, preemph=0.97, remove_dc=True, window=O.povey_window(400), mel_fb=O.mel_filterbank(512, 128),
                                input_scale=scale), float(O.F32_EPS))


@pytest.mark.parametrize("scale", [32768.0, 1.0])
def test_fbank64_matches_the_oracle_on_noise(scale):
    x = synth.noise_clips(2, 16000, seed=0)
    got = O.fbank(x * np.float32(scale))
    e = _fbank64_default(x, scale)
    assert got.shape == e.shape == (2, 98, 128)
    dlog = float(np.abs(got - np.log(e)).max())
    eerr = _energy_err(got, e)
    print(f"fbank noise scale {scale}: max |dlog| {dlog:.3e}, energy-domain {eerr:.3e}")
    assert dlog < 4 * FBANK_LOG_GAP
    assert eerr < 4 * FBANK_ENERGY_GAP


def test_fbank64_matches_the_oracle_on_tones():
    x = synth.tone_clips(16000)
    eerr = _energy_err(O.fbank(x * np.float32(2 ** 15)), _fbank64_default(x, 32768.0))
    print(f"fbank tone: energy-domain {eerr:.3e}")
    assert eerr < 4 * FBANK_TONE_GAP


def test_fbank64_options_against_a_direct_loop():
    """Every option once, one frame at a time with a plain DFT matrix: clip offset, no DC removal, no pre-emphasis, a short window."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 300)).astype(np.float32)
    win, hop, pre = 64, 80, 0.5
    w = rng.uniform(0.1, 1.0, win).astype(np.float32)
    fb = rng.uniform(0.0, 1.0, (257, 5)).astype(np.float32)
    off = np.array([0.25, -0.5], np.float32)
    for dc in (False, True):
        got = F.fbank64(x, win=win, hop=hop, preemph=pre, remove_dc=dc, window=w, mel_fb=fb, input_scale=3.0, clip_offset=off)
        assert got.shape == (2, 3, 5)
        n = np.arange(512)
        dft = np.exp(-2j * np.pi * np.outer(np.arange(257), n) / 512.0)
        for b in range(2):
            for f in range(3):
                s = (x[b, f * hop:f * hop + win].astype(np.float64) - off[b]) * 3.0
                if dc:
                    s = s - s.mean()
                y = np.zeros(512)
                y[:win] = (s - pre * np.concatenate([s[:1], s[:-1]])) * w
                ref = (np.abs(dft @ y) ** 2) @ fb.astype(np.float64)
                assert np.allclose(got[b, f], ref, rtol=1e-10, atol=0)


def test_fbank_helpers():
    img = np.arange(2 * 21 * 40, dtype=np.float64).reshape(2, 21, 40)
    pad = F.fbank_pad(img, 25, norm_mean=2.0, norm_div=4.0)
    assert pad.shape == (2, 25, 40) and np.array_equal(pad[:, :21], img) and (pad[:, 21:] == -0.5).all()
    assert np.array_equal(F.fbank_pad(img, 18), img[:, :18])
    P = 8
    pt = F.cut_patches(img, P)
    nt, nf = 21 // P, 40 // P
    assert pt.shape == (2 * nt * nf, P * P)
    for b, t, f, i, j in ((0, 0, 0, 0, 0), (1, 1, 4, 7, 7), (0, 1, 2, 3, 5), (1, 0, 3, 6, 1)):
        assert pt[(b * nt + t) * nf + f, i * P + j] == img[b, t * P + i, f * P + j]
    assert np.isnan(F.fbank_log(np.array([np.nan, 1.0]), 1e-3)[0])
    assert F.fbank_log(np.array([0.0]), 1e-3)[0] == math.log(float(np.float32(1e-3)))
    assert np.array_equal(F.half_ulp(np.array([1.0, 1.5, 2.0, 0.75]), "f16"), np.array([2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12]))
    assert F.half_ulp(np.array([1.0]), "bf16")[0] == 2.0 ** -8


STFT_CASES = [(96, 24, 96, "hann", True), (400, 160, 400, "hann", True), (800, 160, 800, "hann", True), (2048, 512, 2048, "hann", True),
              (400, 160, 301, "hamming", True), (400, 440, 400, "hann", True), (512, 128, 512, "hann", False), (308, 77, 308, "hann", True)]


@pytest.mark.parametrize("n_fft,hop,win,window,center", STFT_CASES)
def test_stft_power64_matches_torch_stft(n_fft, hop, win, window, center):
    """fp64 against torch.stft in fp64 (tight), and torch.stft in fp32 against the fp64 restatement at the GPU test's PER-FRAME bar on the GPU
    test's inputs (ramped noise): if fp32 torch met it no longer, the inputs would be wrong, not the bar."""
    from avex_amd.kernels import stft_window
    w = stft_window(window, win)
    worst = 0.0
    for T in ((n_fft // 2 + 1, n_fft, 3 * n_fft + 17) if center else (n_fft, n_fft + hop - 1, 3 * n_fft + 17)):
        x = F.ramp_noise(3, T, seed=70)
        ref = F.stft_power64(x, n_fft, hop, win, w, center)
        assert ref.shape == (3, n_fft // 2 + 1, F.stft_frames(T, n_fft, hop, center))
        t64 = torch.stft(torch.from_numpy(x).double(), n_fft=n_fft, hop_length=hop, win_length=win, window=torch.from_numpy(w).double(), center=center,
                         return_complex=True).abs().pow(2).numpy()
        assert np.abs(t64 - ref).max() <= 1e-12 * ref.max()
        t32 = torch.stft(torch.from_numpy(x), n_fft=n_fft, hop_length=hop, win_length=win, window=torch.from_numpy(w), center=center,
                         return_complex=True).abs().pow(2).numpy()
        worst = max(worst, F.per_frame_excess(t32, ref))
    print(f"stft {n_fft}/{hop}/{win}: fp32 torch.stft uses {worst:.3f} of the per-frame bar")
    assert worst <= 1.0


def test_melspec64_matches_the_oracle_and_propagates_nan():
    from avex_amd.kernels import htk_mel_filterbank, stft_window
    x = F.ramp_noise(3, 4000, seed=71)
    mine = F.melspec64(F.stft_power64(x, 400, 160, 400, stft_window("hann", 400), True), htk_mel_filterbank(201, 64, 16000))
    ref = O.audio_processor(x, n_fft=400, hop=160, n_mels=64)
    gap = float(np.abs(mine - ref).max())
    print(f"melspec64 against the fp32 oracle: {gap:.3e}")
    assert mine.shape == ref.shape and gap < 2e-5          # values in [0, 1]; a tenth of the 2e-4 bar the kernels are held to
    assert mine.min() == 0.0 and abs(mine.max() - 1.0) < 1e-6
    # one NaN sample: the reference's amin / amax propagate it, the whole image of that clip is NaN (the oracle does the same)
    bad = x.copy()
    bad[1, 2000] = np.nan
    mine_b = F.melspec64(F.stft_power64(bad, 400, 160, 400, stft_window("hann", 400), True), htk_mel_filterbank(201, 64, 16000))
    with np.errstate(invalid="ignore"):
        ref_b = O.audio_processor(bad, n_fft=400, hop=160, n_mels=64)
    t = torch.log(torch.from_numpy(F.stft_power64(bad, 400, 160, 400, stft_window("hann", 400), True)) + 1e-6)
    assert bool(torch.isnan(t.amin(dim=(1, 2))[1])) and bool(torch.isnan(t.amax(dim=(1, 2))[1]))
    for y in (mine_b, ref_b):
        assert np.isnan(y[1]).all() and np.isfinite(y[0]).all() and np.isfinite(y[2]).all()
    assert np.array_equal(mine_b[0], mine[0]) and np.array_equal(mine_b[2], mine[2])
    # no normalisation: only the frames that hold the sample
    raw = F.melspec64(F.stft_power64(bad, 400, 160, 400, stft_window("hann", 400), True), None, normalize=False)
    holds = np.array([f * 160 - 200 <= 2000 < f * 160 + 200 for f in range(raw.shape[2])])
    assert np.array_equal(np.isnan(raw[1]).any(axis=0), holds) and np.array_equal(np.isnan(raw[1]).all(axis=0), holds)


RATIOS = [(48000, 8000), (16000, 48000), (44100, 48000), (11025, 16000), (44100, 16000), (32000, 16000)]


@pytest.mark.parametrize("orig,new", RATIOS)
def test_resample64_matches_the_oracle(orig, new):
    rng = np.random.default_rng(orig + new)
    for T in (1, 2, 5, 37, 1000):
        x = (rng.standard_normal((2, T)) * 0.3).astype(np.float32)
        ref = IO.resample(x, orig, new)
        got = F.resample64(x, orig, new)
        assert got.shape == ref.shape == (2, math.ceil(T * new / orig))
        assert np.abs(got - ref).max() < 2e-7              # the oracle accumulates in fp64 too: its fp32 result rounding only


def test_resample64_kaiser_window_matches_the_oracle():
    x = (np.random.default_rng(5).standard_normal((1, 500)) * 0.3).astype(np.float32)
    assert np.abs(F.resample64(x, 44100, 16000, beta=14.769656459379492) - IO.resample(x, 44100, 16000, beta=14.769656459379492)).max() < 2e-7


@pytest.mark.parametrize("orig,new", RATIOS)
def test_resample_interp64_matches_the_oracle(orig, new):
    """The oracle keeps its table in fp64, the restatement rounds it to fp32 like the device: 2^-24 relative per weight, far below 5e-7."""
    rng = np.random.default_rng(orig * 3 + new)
    for T in (1, 2, 5, 37, 700):
        x = (rng.standard_normal((2, T)) * 0.3).astype(np.float32)
        got = F.resample_interp64(x, orig, new)
        assert got.shape == (2, math.ceil(T * new / orig))
        for b in range(2):
            ref = IO.resample_librosa(x[b], orig, new)
            assert ref.shape == got[b].shape
            assert np.abs(got[b] - ref).max() < 5e-7
    assert np.array_equal(F.resample_interp64(x, orig, new, scale=False), F.resample_interp64(x, orig, new) * math.sqrt(new / orig)) or \
        np.allclose(F.resample_interp64(x, orig, new, scale=False), F.resample_interp64(x, orig, new) * math.sqrt(new / orig), rtol=1e-14, atol=0)


@pytest.mark.parametrize("G,T", [(1, 1), (3, 65), (2, 200)])
def test_posconv64_matches_torch_and_the_oracle(G, T):
    cg, K = 48, 128
    E = cg * G
    x = synth.normal(f"frx{G}{T}", (2, T, E), 1.0)
    w = synth.normal("frw", (E, cg, K), math.sqrt(1.0 / (K * cg)))
    bias = synth.normal("frb", (E,), 0.05)
    res = synth.normal("frr", (2, T, E), 1.0)
    out, conv = F.posconv64(x, w, bias, G, residual=res)
    t = torch.nn.functional.conv1d(torch.from_numpy(x).double().transpose(1, 2), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                                   padding=K // 2, groups=G)[:, :, :-1]
    t = torch.nn.functional.gelu(t).transpose(1, 2).numpy()
    assert conv.shape == t.shape == (2, T, E)
    assert np.abs(conv - t).max() < 1e-12
    assert np.array_equal(out, res.astype(np.float64) + conv)
    assert np.array_equal(F.posconv64(x, w, bias, G)[0], x.astype(np.float64) + conv)
    o32 = O.pos_conv(x, w, bias, G)
    assert np.linalg.norm(o32 - conv) / np.linalg.norm(conv) < 2e-6
