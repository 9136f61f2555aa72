"""NumPy restatement of avex_amd.measurements for the tests: the frames of a box, its spectrum and envelope, and the measurements.

Written from the description, not from the package's code: loops over frames and bins where the package uses closed forms and kernels.
Frames, the window and the float64 transform are those of tests/_activity_ref.py; the float32 CPU chain is tests/_soundscape_ref.power32.

  box           samples [s0, s1) of a recording, bins [lo, hi); its frames are the f with f hop >= s0 and f hop + 512 <= s1 that the
                recording has: f0 the first of them, n their number
  statistics    spectrum[k] = sum over the box's frames of P[f, k] inside the band, 0 outside; envelope[t] = sum over the band of
                P[f0 + t, k]; nonfinite = the NaN frames; with one, spectrum is NaN inside the band
  measurements  S' = max(spectrum - n noise, 0), e' = max(envelope - sum_band noise, 0) (without noise: spectrum, envelope); the
                quantile index of level q over v = the smallest i with cumsum(v)[i] >= q sum(v); levels (1 - p) / 2, 0.5, 1 - (1 - p) / 2;
                the columns as the docstring of avex_amd/measurements.py defines them
"""
import math

import numpy as np

import _activity_ref as A

N_BINS = 257
INTS = ("n_frames", "nonfinite", "low_bin", "centre_bin", "high_bin", "peak_bin", "low_frame", "centre_frame", "high_frame", "peak_frame")
FLOATS = ("energy", "snr_db", "low_hz", "centre_hz", "high_hz", "peak_hz", "bandwidth_hz", "begin_s", "end_s", "centre_s", "peak_s", "duration_s")
# the inputs of the decision tests: boxes in samples of A.synthetic(), bands in bins
BOXES = ((16000, 25600), (64000, 96000), (0, 96123), (51200, 52000), (40000, 60000), (8000, 40000))
BANDS = ((0, 257), (64, 256), (32, 129))
P_DEFAULT = 0.9


def event_frames(s0, s1, hop, n_samples):
    """(f0, n) by counting: the frames of the recording wholly inside [s0, s1)."""
    inside = [f for f in range(A.n_frames_of(n_samples, hop)) if f * hop >= s0 and f * hop + A.N_FFT <= s1]
    f0 = 0
    while f0 * hop < s0:
        f0 += 1
    return f0, len(inside)


def levels(p):
    q = (1.0 - p) / 2.0
    return q, 0.5, 1.0 - q


def stats_of_power(P, f0, n, lo, hi):
    """P: [F, 257] of any float dtype (NaN rows for non-finite frames) -> (spectrum [257], envelope [n], nonfinite); sums in the dtype of P."""
    rows = P[f0:f0 + n]
    spectrum = np.zeros(N_BINS, P.dtype)
    bad = int(np.isnan(rows[:, 0]).sum()) if n else 0
    if n:
        spectrum[lo:hi] = np.nan if bad else rows[:, lo:hi].sum(axis=0, dtype=P.dtype)
    envelope = rows[:, lo:hi].sum(axis=1, dtype=P.dtype) if n else np.zeros(0, P.dtype)
    return spectrum, envelope, bad


def quantile_index(v, q):
    """The smallest i with cumsum(v)[i] >= q sum(v), and the margin min |C_i - q E| / E at that index and the one before."""
    C = np.cumsum(np.asarray(v, dtype=np.float64))
    E = C[-1]
    i = 0
    while not C[i] >= q * E:
        i += 1
    margin = min(abs(C[j] - q * E) for j in (i, i - 1) if j >= 0) / E
    return i, margin


def measure(spectrum, envelope, nonfinite, f0, lo, hi, hop, sr, p=P_DEFAULT, noise=None):
    """One event from its statistics (any float dtype) -> a dict of every column, and under "margins" the six quantile margins."""
    n = len(envelope)
    out = {k: -1 for k in INTS}
    out.update({k: math.nan for k in FLOATS})
    out["n_frames"], out["nonfinite"], out["margins"] = n, int(nonfinite), []
    if n == 0 or nonfinite > 0:
        return out
    S = np.asarray(spectrum, dtype=np.float64)[lo:hi]
    e = np.asarray(envelope, dtype=np.float64)
    if noise is not None:
        nz = np.asarray(noise, dtype=np.float64)[lo:hi]
        band = 0.0
        for v in nz:
            band += v
        d, de = S - n * nz, e - band
        S, e = np.where(d <= 0.0, 0.0, d), np.where(de <= 0.0, 0.0, de)
    E = float(np.cumsum(S)[-1])
    out["energy"] = E
    if noise is not None and n * band != 0.0:
        with np.errstate(divide="ignore"):
            out["snr_db"] = float(10.0 * np.log10(np.float64(E) / (n * band)))
    bin_hz = sr / 512.0
    if E > 0.0:
        for name, q in zip(("low", "centre", "high"), levels(p)):
            i, m = quantile_index(S, q)
            out[f"{name}_bin"], out[f"{name}_hz"] = lo + i, (lo + i) * bin_hz
            out["margins"].append(m)
        out["peak_bin"] = lo + int(np.argmax(S))                       # the lowest index attaining the maximum
        out["peak_hz"] = out["peak_bin"] * bin_hz
        out["bandwidth_hz"] = out["high_hz"] - out["low_hz"] + bin_hz
    if float(np.cumsum(e)[-1]) > 0.0:
        for name, q in zip(("low", "centre", "high"), levels(p)):
            i, m = quantile_index(e, q)
            out[f"{name}_frame"] = f0 + i
            out["margins"].append(m)
        out["peak_frame"] = f0 + int(np.argmax(e))
        out["begin_s"] = out["low_frame"] * hop / sr
        out["end_s"] = (out["high_frame"] * hop + 512) / sr
        out["centre_s"] = (out["centre_frame"] * hop + 256) / sr
        out["peak_s"] = (out["peak_frame"] * hop + 256) / sr
        out["duration_s"] = out["end_s"] - out["begin_s"]
    return out


def measure_box(P, s0, s1, lo, hi, hop, sr, n_samples, p=P_DEFAULT, noise=None):
    """The whole chain for one box from the power rows P of its recording."""
    f0, n = event_frames(s0, s1, hop, n_samples)
    spectrum, envelope, bad = stats_of_power(P, f0, n, lo, hi)
    out = measure(spectrum, envelope, bad, f0, lo, hi, hop, sr, p, noise)
    out["spectrum"], out["envelope"], out["first_frame"] = spectrum, envelope, f0
    return out


def deviations(spectrum, envelope, ref_spectrum, ref_envelope, P64, f0, n):
    """(max |spectrum - ref| / sum_t P_f, max |envelope - ref| / P_f), P_f the frame's total power (all bins) in float64."""
    pf = P64[f0:f0 + n].sum(axis=1)
    d_s = float(np.max(np.abs(np.asarray(spectrum, dtype=np.float64) - ref_spectrum))) / float(pf.sum())
    d_e = float(np.max(np.abs(np.asarray(envelope, dtype=np.float64) - ref_envelope) / pf))
    return d_s, d_e


def noise_spectrum(mean_power, n_frames, nonfinite, recording, S, n_rec):
    """[n_rec, 257]: per recording the minimum of mean_power over its full segments without a non-finite frame; NaN where none."""
    out = np.full((n_rec, N_BINS), np.nan, dtype=np.float32)
    for r in range(n_rec):
        rows = [mean_power[g] for g in range(len(n_frames)) if recording[g] == r and n_frames[g] == S and nonfinite[g] == 0]
        if rows:
            out[r] = np.min(np.stack(rows), axis=0)
    return out
