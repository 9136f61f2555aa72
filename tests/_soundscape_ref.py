"""NumPy float64 restatement of avex_amd.soundscape for the tests: per-segment spectral statistics and the eight acoustic indices.

Written from the description, not from the package's code: loops over segments, frames and bands where the package uses tables and
kernels.  Frames, the window and the float64 transform are those of tests/_activity_ref.py.

  frames      n_fft = 512, periodic Hann (float64 -> float32), F = (n - 512) // hop + 1 frames (0 when n < 512), P[t, k] = |X_t[k]|^2 for
              k = 0 .. 256, A = sqrt(P); P_FS = 16384; a frame holding a NaN or an Inf is NaN in every bin
  segments    segment g = frames [g S, min((g + 1) S, F)); its span in seconds runs from its first frame's first sample to its last
              frame's last sample
  statistics  mean_power = sum P / n, mean_amplitude = sum A / n, abs_diff = sum_{t >= 1} |A[t] - A[t-1]| inside the segment,
              count_above = #{t: P > float32(P_FS 10^(db / 10))} (strict); with a non-finite frame the three float statistics are NaN in
              every bin and count_above counts the finite frames
  indices     aci, adi, aei, bi, ndsi, hf, ht, h as the docstring of avex_amd/soundscape.py defines them; all NaN with a non-finite frame
"""
import math

import numpy as np

import _activity_ref as A

P_FS = 16384.0
N_BINS = 257
NAMES = ("aci", "adi", "aei", "bi", "ndsi", "hf", "ht", "h")


class Spec:
    """The fields of an IndexSpec the restatement reads (any object with these attributes serves)."""

    def __init__(self, band=None, bio_band=(2000.0, 8000.0), anthro_band=(1000.0, 2000.0), adi_step_hz=1000.0, adi_max_hz=10000.0):
        self.band, self.bio_band, self.anthro_band, self.adi_step_hz, self.adi_max_hz = band, bio_band, anthro_band, adi_step_hz, adi_max_hz


def threshold(db_threshold):
    with np.errstate(over="ignore"):
        return np.float32(np.float64(P_FS) * np.float64(10.0) ** (np.float64(db_threshold) / 10.0))


def segments_of(n_frames, S):
    """[(first frame, frames)] of a recording of n_frames frames."""
    out, f = [], 0
    while f < n_frames:
        out.append((f, min(S, n_frames - f)))
        f += S
    return out


def spans_s(n_samples, hop, S, sr):
    """[(start_s, end_s)] of the segments of a recording of n_samples samples."""
    return [(f * hop / sr, ((f + n - 1) * hop + A.N_FFT) / sr) for f, n in segments_of(A.n_frames_of(n_samples, hop), S)]


def stats_of_power(P, S, db_threshold):
    """P: [F, 257] of any float dtype (NaN rows for non-finite frames); sums in the dtype of P."""
    thr = threshold(db_threshold)
    amp = np.sqrt(P)
    segs = segments_of(len(P), S)
    G = len(segs)
    out = {"mean_power": np.zeros((G, N_BINS), P.dtype), "mean_amplitude": np.zeros((G, N_BINS), P.dtype), "abs_diff": np.zeros((G, N_BINS), P.dtype),
           "count_above": np.zeros((G, N_BINS), np.int32), "n_frames": np.zeros(G, np.int32), "nonfinite_frames": np.zeros(G, np.int32),
           "frame_power": P.sum(axis=1, dtype=P.dtype) if len(P) else np.zeros(0, P.dtype), "first_frame": np.zeros(G, np.int64)}
    for g, (f, n) in enumerate(segs):
        rows, arows = P[f:f + n], amp[f:f + n]
        bad = int(np.isnan(rows[:, 0]).sum())
        out["n_frames"][g], out["nonfinite_frames"][g], out["first_frame"][g] = n, bad, f
        with np.errstate(invalid="ignore"):
            out["count_above"][g] = (rows > thr).sum(axis=0)                       # a NaN is not above
        if bad:
            out["mean_power"][g] = out["mean_amplitude"][g] = out["abs_diff"][g] = np.nan
            continue
        out["mean_power"][g] = rows.sum(axis=0, dtype=P.dtype) / P.dtype.type(n)
        out["mean_amplitude"][g] = arows.sum(axis=0, dtype=P.dtype) / P.dtype.type(n)
        if n > 1:
            out["abs_diff"][g] = np.abs(arows[1:] - arows[:-1]).sum(axis=0, dtype=P.dtype)
    return out


def stats64(x, hop, S, db_threshold):
    return stats_of_power(A.frame_power64(x, hop), S, db_threshold)


def power32(x, hop):
    """[F, 257] float32: the float32 CPU chain -- torch.fft.rfft of the float32 product, float32 |.|^2; NaN rows for non-finite frames."""
    import torch
    F = A.n_frames_of(len(x), hop)
    if F == 0:
        return np.zeros((0, N_BINS), np.float32)
    frames = np.stack([x[f * hop:f * hop + A.N_FFT] for f in range(F)]).astype(np.float32)
    X = torch.fft.rfft(torch.from_numpy(frames * A.hann()))
    P = (X.real ** 2 + X.imag ** 2).numpy()
    P[~np.isfinite(frames).all(axis=1)] = np.nan
    return P


def stats32(x, hop, S, db_threshold):
    """The same statistics from the float32 CPU chain with float32 sqrt and sums: the yardstick of the device's deviation."""
    return stats_of_power(power32(x, hop), S, db_threshold)


def adi_bands(spec, sr):
    J = int(math.floor(min(spec.adi_max_hz, sr / 2.0) / spec.adi_step_hz))
    assert 1 <= J <= 32, J
    return [(j * spec.adi_step_hz, (j + 1) * spec.adi_step_hz) for j in range(J)]


def _xlogx(q):
    return q * math.log(q) if q > 0.0 else 0.0


def indices(stats, frame_power, n, spec, sr):
    """One segment.  stats: a mapping with mean_power, mean_amplitude, abs_diff, count_above ([257] each, any dtype) and optionally
    nonfinite_frames; frame_power: the segment's n frame powers.  -> [8] float64 in the order of NAMES."""
    if int(stats.get("nonfinite_frames", 0)) > 0:
        return np.full(8, np.nan)
    mp = np.asarray(stats["mean_power"], dtype=np.float64)
    ma = np.asarray(stats["mean_amplitude"], dtype=np.float64)
    ad = np.asarray(stats["abs_diff"], dtype=np.float64)
    ca = np.asarray(stats["count_above"], dtype=np.int64)
    fp = np.asarray(frame_power, dtype=np.float64)
    assert mp.shape == (N_BINS,) and len(fp) == n
    (b_lo, b_hi), = A.bins([spec.band], sr) if spec.band is not None else [(0, N_BINS)]
    (bio_lo, bio_hi), (an_lo, an_hi) = A.bins([spec.bio_band, spec.anthro_band], sr)

    aci = 0.0
    for k in range(b_lo, b_hi):
        if ma[k] != 0.0:
            aci += ad[k] / (n * ma[k])

    p = [float(ca[lo:hi].sum()) / (n * (hi - lo)) for lo, hi in A.bins(adi_bands(spec, sr), sr)]
    J, sp = len(p), math.fsum(p)
    if sp > 0.0:
        adi = -math.fsum(_xlogx(pj / sp) for pj in p)
        aei = math.fsum(abs(pi - pj) for pi in p for pj in p) / (2.0 * J * sp)
    else:
        adi = aei = math.nan

    L = [10.0 * math.log10(max(mp[k], 1e-12 * P_FS) / P_FS) for k in range(bio_lo, bio_hi)]
    bi = math.fsum(v - min(L) for v in L) * (sr / 512.0) / 1000.0

    b, a = math.fsum(mp[bio_lo:bio_hi]), math.fsum(mp[an_lo:an_hi])
    ndsi = (b - a) / (b + a) if a + b != 0.0 else math.nan

    total, K = math.fsum(mp[b_lo:b_hi]), b_hi - b_lo
    hf = -math.fsum(_xlogx(mp[k] / total) for k in range(b_lo, b_hi)) / math.log(K) if total > 0.0 and K >= 2 else math.nan

    t_total = math.fsum(fp)
    ht = -math.fsum(_xlogx(v / t_total) for v in fp) / math.log(n) if t_total > 0.0 and n >= 2 else math.nan
    return np.array([aci, adi, aei, bi, ndsi, hf, ht, hf * ht], dtype=np.float64)


def indices_of(stats, spec, sr):
    """[G, 8]: indices() over every segment of a stats_of_power() result."""
    G = len(stats["n_frames"])
    out = np.zeros((G, 8))
    for g in range(G):
        f, n = int(stats["first_frame"][g]), int(stats["n_frames"][g])
        seg = {k: stats[k][g] for k in ("mean_power", "mean_amplitude", "abs_diff", "count_above", "nonfinite_frames")}
        out[g] = indices(seg, stats["frame_power"][f:f + n], n, spec, sr)
    return out


def deviations(got, ref64):
    """The three deviations of the issue, each the maximum over segments and bins: |mean_power - ref| / mean_t(P_f),
    |mean_amplitude - ref| / mean_t(sqrt(P_f)), |abs_diff - ref| / ((n - 1) mean_t(sqrt(P_f))), P_f the frame's total power in float64.
    Segments with a non-finite frame are left out (compared elsewhere); a one-frame segment has no abs_diff term."""
    d = [0.0, 0.0, 0.0]
    for g in range(len(ref64["n_frames"])):
        if ref64["nonfinite_frames"][g]:
            continue
        f, n = int(ref64["first_frame"][g]), int(ref64["n_frames"][g])
        pf = ref64["frame_power"][f:f + n]
        m_p, m_a = float(pf.mean()), float(np.sqrt(pf).mean())
        if m_p == 0.0:
            continue
        d[0] = max(d[0], float(np.max(np.abs(got["mean_power"][g].astype(np.float64) - ref64["mean_power"][g]))) / m_p)
        d[1] = max(d[1], float(np.max(np.abs(got["mean_amplitude"][g].astype(np.float64) - ref64["mean_amplitude"][g]))) / m_a)
        if n > 1:
            d[2] = max(d[2], float(np.max(np.abs(got["abs_diff"][g].astype(np.float64) - ref64["abs_diff"][g]))) / ((n - 1) * m_a))
    return d


def count_allowance(P64, P32, S, db_threshold):
    """(allowance [G, 257], bar): the cells of each (segment, bin) with |P64 - thr| <= bar * P_f, bar = 8 x max |P32 - P64| / P_f."""
    thr = float(threshold(db_threshold))
    pf = P64.sum(axis=1, keepdims=True)
    bar = 8.0 * float(np.max(np.abs(P32.astype(np.float64) - P64) / pf))
    near = np.abs(P64 - thr) <= bar * pf
    return np.stack([near[f:f + n].sum(axis=0) for f, n in segments_of(len(P64), S)]), bar
