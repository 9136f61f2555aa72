"""NumPy restatement of avex_amd.recordings for the tests: the window plan, rows and masks, statistics and the gate.

Written from the description (windows start at 0, hop, 2 hop, ... while start < n; a row is the samples, then zeros, mask True on the
zeros; energy = sum x^2 in float64, peak = max |x|; a window is kept iff valid > 0, energy >= thr_energy * valid and peak >= thr_peak),
not from the package's code: loops where the package uses closed forms.
"""
import numpy as np


def plan(n_samples, window_len, hop_len, tail="pad"):
    if n_samples <= 0 or window_len <= 0 or hop_len <= 0:
        raise ValueError("positive lengths expected")
    if tail not in ("pad", "drop"):
        raise ValueError(f"unknown tail {tail!r}")
    starts, valids = [], []
    s = 0
    while s < n_samples:
        v = min(window_len, n_samples - s)
        if tail == "pad" or v == window_len:
            starts.append(s)
            valids.append(v)
        s += hop_len
    if not starts:                       # tail="drop" on a recording shorter than one window
        starts, valids = [0], [n_samples]
    return starts, valids


def rows(x, starts, valids, window_len):
    """(wav [B, window_len] float32, mask [B, window_len] bool) of a 1-d float32 waveform."""
    wav = np.zeros((len(starts), window_len), dtype=np.float32)
    mask = np.ones((len(starts), window_len), dtype=bool)
    for b, (s, v) in enumerate(zip(starts, valids)):
        wav[b, :v] = x[s:s + v]
        mask[b, :v] = False
    return wav, mask


def stats(x, starts, valids):
    """(energy float64, peak float32) per window; a window holding a NaN or an Inf has NaN for both."""
    energy, peak = np.zeros(len(starts), dtype=np.float64), np.zeros(len(starts), dtype=np.float32)
    for b, (s, v) in enumerate(zip(starts, valids)):
        seg = x[s:s + v]
        if not np.isfinite(seg).all():
            energy[b], peak[b] = np.nan, np.nan
            continue
        energy[b] = np.sum(seg.astype(np.float64) ** 2)
        peak[b] = np.abs(seg).max() if v else 0.0
    return energy, peak


def db(energy, peak, valids):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(energy / np.asarray(valids, dtype=np.float64)), 20.0 * np.log10(peak.astype(np.float64))


def thresholds(min_rms_db=None, min_peak_db=None):
    """(thr_energy as a mean square, thr_peak as an amplitude); None -> -inf (off)."""
    return (-np.inf if min_rms_db is None else 10.0 ** (min_rms_db / 10.0), -np.inf if min_peak_db is None else 10.0 ** (min_peak_db / 20.0))


def select(energy, peak, valids, thr_energy=-np.inf, thr_peak=-np.inf):
    kept = []
    for w, (e, p, v) in enumerate(zip(energy, peak, valids)):
        if v > 0 and e >= thr_energy * v and p >= thr_peak:      # NaN fails both compares
            kept.append(w)
    return kept
