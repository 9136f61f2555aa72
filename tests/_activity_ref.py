"""NumPy restatement of avex_amd.activity for the tests: frames, band energies in float64, the noise floor, active frames, the gate.

Written from the description, not from the package's code: loops and a sort where the package uses closed forms and a radix select.

  frames      n_fft = 512; a recording of n samples has (n - 512) // hop + 1 frames (0 when n < 512), frame f = samples [f hop, f hop + 512)
  energy      y = x * w (w the periodic Hann table, float64 -> float32), X = DFT(y), E[b, f] = sum of |X[k]|^2 over k_lo <= k < k_hi,
              k_lo = ceil(lo 512 / sr), k_hi = min(ceil(hi 512 / sr), 257); a frame holding a NaN or an Inf is NaN in every band
  floor       the float32 energy whose bit pattern (uint32) has rank floor(p / 100 (F - 1)) in ascending order; NaN when F = 0
  active      E > float32(max(floor, floor_min) * ratio), ratio = float32(10^(snr_db / 10)), floor_min = float32(10^(min_floor_db / 10)) or 0
  window      frames ceil(start / hop) .. floor((start + valid - 512) / hop); n_frames, active_frames, max_energy (NaN if any, -inf if none)
  gate        the level conditions of tests/_recordings_ref.select and active_frames >= min_active_frames in any / every band
"""
import math

import numpy as np

N_FFT = 512
SR = 16000
N_SYNTH = 6 * SR + 123
BANDS = ((2000.0, 4000.0), (6000.0, 8000.0), (0.0, 8001.0))
SNR_DB = 10.0
PERCENTILE = 20.0
HOPS = (256, 200)
MARGIN = 0.05                 # no frame energy of the synthetic input lies this close to its threshold (asserted in test_activity_cpu.py)


def hann():
    n = np.arange(N_FFT, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)).astype(np.float32)


def synthetic(seed=0):
    """6 s + 123 samples at 16 kHz, float32: -40 dBFS Gaussian noise (RMS 0.01) and -10 dBFS tone bursts (amplitude 10^-0.5): 3 kHz over
    1.0-1.6 s and 3.2-3.25 s, 6.5 kHz over 4.5-5.2 s."""
    rng = np.random.default_rng(seed)
    x = 0.01 * rng.standard_normal(N_SYNTH)
    t = np.arange(N_SYNTH, dtype=np.float64) / SR
    amp = 10.0 ** (-10.0 / 20.0)
    for hz, t0, t1 in ((3000.0, 1.0, 1.6), (3000.0, 3.2, 3.25), (6500.0, 4.5, 5.2)):
        on = (t >= t0) & (t < t1)
        x[on] += amp * np.sin(2.0 * np.pi * hz * t[on])
    return x.astype(np.float32)


def bins(bands, sr):
    out = []
    for lo, hi in bands:
        k_lo, k_hi = math.ceil(lo * N_FFT / sr), min(math.ceil(hi * N_FFT / sr), N_FFT // 2 + 1)
        assert 0 <= k_lo < k_hi, (lo, hi)
        out.append((k_lo, k_hi))
    return out


def n_frames_of(n_samples, hop):
    count, f = 0, 0
    while f * hop + N_FFT <= n_samples:
        count, f = count + 1, f + 1
    return count


def frame_power64(x, hop):
    """[F, 257] float64: |rfft|^2 of the float64 product of the float32 samples and the float32 table; NaN rows for non-finite frames."""
    w = hann().astype(np.float64)
    F = n_frames_of(len(x), hop)
    P = np.zeros((F, N_FFT // 2 + 1), dtype=np.float64)
    for f in range(F):
        seg = x[f * hop:f * hop + N_FFT]
        if not np.isfinite(seg).all():
            P[f] = np.nan
            continue
        X = np.fft.rfft(seg.astype(np.float64) * w)
        P[f] = X.real ** 2 + X.imag ** 2
    return P


def band_energy(P, kbins):
    """[n_bands, F] in the dtype of P."""
    return np.stack([P[:, lo:hi].sum(axis=1) for lo, hi in kbins]) if len(P) else np.zeros((len(kbins), 0), dtype=P.dtype)


def floor_rank(n_frames, percentile):
    return int(math.floor(percentile / 100.0 * (n_frames - 1))) if n_frames > 0 else 0


def key_sorted(e32):
    """The float32 energies of one (recording, band) in ascending order of their bit patterns."""
    keys = np.sort(np.ascontiguousarray(e32, dtype=np.float32).view(np.uint32))
    return keys.view(np.float32)


def noise_floor(e32, percentile, shift=0):
    """float32 floor of one (recording, band); ``shift`` moves the rank by that many places (clamped), for the margin check."""
    if len(e32) == 0:
        return np.float32(np.nan)
    r = min(max(floor_rank(len(e32), percentile) + shift, 0), len(e32) - 1)
    return key_sorted(e32)[r]


def nonfinite_count(e32):
    return int(np.isnan(np.asarray(e32, dtype=np.float32)).sum())


def ratio_of(snr_db):
    return np.float32(10.0 ** (snr_db / 10.0))


def floor_min_of(min_floor_db):
    return np.float32(0.0) if min_floor_db is None else np.float32(10.0 ** (min_floor_db / 10.0))


def threshold(floor, snr_db, min_floor_db=None):
    with np.errstate(invalid="ignore"):
        return np.float32(np.maximum(np.float32(floor), floor_min_of(min_floor_db)) * ratio_of(snr_db))      # NaN stays NaN; float32 * float32


def window_frames(start, valid, hop):
    """The frames (numbers inside the recording) that lie wholly inside [start, start + valid)."""
    return [f for f in range(0, (start + valid) // hop + 1) if f * hop >= start and f * hop + N_FFT <= start + valid]


def window_stats(e32, floors, starts, valids, hop, snr_db, min_floor_db=None):
    """One recording: e32 [n_bands, F] float32, floors [n_bands] -> (n_frames [W], active [W, n_bands] int32, max_energy [W, n_bands] float32)."""
    nb = e32.shape[0]
    n_frames = np.zeros(len(starts), dtype=np.int32)
    active = np.zeros((len(starts), nb), dtype=np.int32)
    mx = np.full((len(starts), nb), -np.inf, dtype=np.float32)
    for w, (s, v) in enumerate(zip(starts, valids)):
        fr = window_frames(int(s), int(v), hop)
        n_frames[w] = len(fr)
        for b in range(nb):
            thr = threshold(floors[b], snr_db, min_floor_db)
            vals = e32[b, fr]
            with np.errstate(invalid="ignore"):
                active[w, b] = int((vals > thr).sum())            # a NaN on either side: not active
            if len(fr):
                mx[w, b] = np.max(vals)                           # np.max keeps a NaN
    return n_frames, active, mx


def band_condition(active, min_active_frames, mode):
    ok = active >= min_active_frames
    return ok.any(axis=1) if mode == "any" else ok.all(axis=1)


def kept_list(level_kept, active, min_active_frames, mode):
    """``level_kept``: the windows tests/_recordings_ref.select keeps; the gate's list, in increasing order."""
    cond = band_condition(active, min_active_frames, mode)
    return [w for w in level_kept if cond[w]]


def analyse(x, starts, valids, hop, kbins, snr_db=SNR_DB, percentile=PERCENTILE, min_floor_db=None, energy32=None):
    """The whole chain for one recording.  ``energy32``: float32 [n_bands, F] to decide from (the device's own); ``None``: the float64
    reference rounded to float32."""
    if energy32 is None:
        energy32 = band_energy(frame_power64(x, hop), kbins).astype(np.float32)
    floors = np.array([noise_floor(energy32[b], percentile) for b in range(len(kbins))], dtype=np.float32)
    n_frames, active, mx = window_stats(energy32, floors, starts, valids, hop, snr_db, min_floor_db)
    return {"energy": energy32, "floor": floors, "nonfinite": nonfinite_count(energy32[0]) if energy32.shape[1] else 0, "n_frames": n_frames,
            "active_frames": active, "max_energy": mx}


def closest_approach(e32, percentile, snr_db):
    """min over bands, frames and rank shifts -1, 0, +1 of |E - thr| / thr, for the margin assertion."""
    best = np.inf
    for b in range(e32.shape[0]):
        for shift in (-1, 0, 1):
            thr = threshold(noise_floor(e32[b], percentile, shift), snr_db)
            best = min(best, float(np.min(np.abs(e32[b].astype(np.float64) - float(thr)) / float(thr))))
    return best
