"""Acoustic indices over recordings: what each stretch of a soundscape looks like, before any model is chosen.

Every other step of the package asks what called, and when.  This one gives the answers an ecologist reads first: the long-term average
spectrum of each minute and the standard indices over it -- Acoustic Complexity, Diversity and Evenness, the Bioacoustic Index, NDSI,
spectral and temporal entropy -- from the waveform a :class:`~avex_amd.recordings.RecordingWindows` already holds on the device.  Three
kernels of ``csrc/soundscape.hip``; there is no CPU fallback.

Semantics (the tests hold them; ``tests/_soundscape_ref.py`` restates them in NumPy float64):

* **Frames** as in :mod:`avex_amd.activity`: ``n_fft = 512``, the periodic Hann table in fp32 (``activity.tables()``), ``hop`` 32..512;
  recording ``r`` of ``n_r`` samples has ``F_r = (n_r - 512) // hop + 1`` frames (0 when ``n_r < 512``), no padding.  ``P[t, k] = |X_t[k]|^2``
  for ``k = 0..256`` and ``A = sqrt(P)``, fp32.  Full scale is ``P_FS = 16384``: a full-scale sine on a bin has ``|X| = 128`` under this
  window.  A frame's ``P[t, :]`` is a function of that frame's 512 samples alone (one frame per transform).  A frame of zeros gives ``+0``
  in every bin, a frame holding a NaN or an Inf NaN in every bin.
* **Segments.**  ``segment_frames = S = round(segment_s * sr / hop) >= 1``; segment ``g`` of recording ``r`` holds its frames
  ``[g S, min((g + 1) S, F_r))``, ``G_r = ceil(F_r / S)``; a short last segment is reported with its own ``n_frames``.  The segments of all
  recordings lie back to back, ``segment_ranges[r] = [g0, g1)``.  ``start_s`` / ``end_s``: from the first frame's first sample to the last
  frame's last sample.
* **Statistics** per (segment, bin) over the segment's ``n`` frames in time order: ``mean_power = sum P / n``, ``mean_amplitude = sum A / n``,
  ``abs_diff = sum_{t >= 1} |A[t] - A[t-1]|`` inside the segment (0 when ``n = 1``), ``count_above`` = the frames with ``P > thr`` (strict,
  fp32), ``thr = fl32(P_FS * 10^(db_threshold / 10))`` (``-inf``: 0, ``+inf``: no cell).  ``frame_power[f]`` = the sum of ``P[f, :]``;
  ``nonfinite_frames[g]``.  A segment with a non-finite frame has NaN in its three float statistics, in every bin; its ``count_above``
  counts the finite frames.  A segment's numbers depend on its recording's samples, ``hop``, ``S`` and ``db_threshold`` alone: the same
  bits in any company and on every run.
* **Indices** per segment, float64 on the device from those fp32 statistics, in the order of :data:`INDEX_NAMES`.  Bands are
  ``(lo_hz, hi_hz)`` turned into bins by :func:`avex_amd.activity.band_bins`; ``band = None`` is all 257 bins; the ADI bands are
  ``[j step, (j + 1) step)`` for ``j < J = floor(min(adi_max_hz, sr / 2) / adi_step_hz)``, ``1 <= J <= 32``.

  ``aci``   sum over ``band`` of ``abs_diff / (n mean_amplitude)``; bins with ``mean_amplitude == 0`` add 0
  ``adi``   ``p_j = (sum of count_above over band j) / (n bins_j)``, ``q_j = p_j / sum p``: ``-sum q ln q`` (``q = 0`` adds 0)
  ``aei``   ``sum_i sum_j |p_i - p_j| / (2 J sum p)`` (the Gini coefficient); ``adi`` and ``aei`` are NaN when ``sum p = 0``
  ``bi``    ``L_k = 10 log10(max(mean_power, 1e-12 P_FS) / P_FS)`` over ``bio_band``: ``sum (L_k - min L) * (sr / 512) / 1000``, dB kHz
  ``ndsi``  ``(b - a) / (b + a)``, the sums of ``mean_power`` over ``bio_band`` and ``anthro_band``; NaN when ``a + b = 0``
  ``hf``    ``q_k = mean_power / its sum over band``: ``-sum q ln q / ln K``; NaN when the sum is 0 or ``K < 2``
  ``ht``    ``q_t = frame_power / its sum over the segment``: ``-sum q ln q / ln n``; NaN when the sum is 0 or ``n < 2``
  ``h``     ``hf * ht``

  Every column is NaN for a segment with a non-finite frame.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi, activity
from ._capi import check, lib
from ._frames import N_BINS, N_FFT, _number, _tables_on, _to_device, frame_count, recording_table

__all__ = ["IndexSpec", "SpectralStats", "SoundscapeIndices", "spectral_stats", "acoustic_indices", "acoustic_indices_of", "segment_plan", "INDEX_NAMES",
           "P_FS"]

P_FS = 16384.0                            # AVEXHIP_SOUNDSCAPE_FULL_SCALE
RUN_FRAMES = 64                           # AVEXHIP_SOUNDSCAPE_RUN_FRAMES
MAX_SEGMENT_FRAMES = 1 << 24              # AVEXHIP_SOUNDSCAPE_MAX_SEGMENT_FRAMES
MAX_ADI_BANDS = 32                        # AVEXHIP_SOUNDSCAPE_MAX_ADI_BANDS
INDEX_NAMES = ("aci", "adi", "aei", "bi", "ndsi", "hf", "ht", "h")
# avexhip_soundscape_recording and avexhip_soundscape_index_spec, field for field
RECORDING_DTYPE = np.dtype([("base", "<i8"), ("n_samples", "<i8"), ("first_frame", "<i8"), ("first_segment", "<i4"), ("first_run", "<i4")])
INDEX_SPEC_DTYPE = np.dtype([("band", "<i4", (2,)), ("bio", "<i4", (2,)), ("anthro", "<i4", (2,)), ("n_adi", "<i4"), ("reserved", "<i4"),
                             ("adi", "<i4", (MAX_ADI_BANDS, 2)), ("bin_khz", "<f8")])


def _band(x: Any, what: str) -> Tuple[float, float]:
    try:
        lo, hi = x
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}={x!r}: a (lo_hz, hi_hz) pair expected") from e
    lo, hi = _number(lo, what), _number(hi, what)
    if not 0.0 <= lo < hi:
        raise ValueError(f"{what} ({lo}, {hi}): 0 <= lo_hz < hi_hz expected")
    return lo, hi


@dataclass(frozen=True)
class IndexSpec:
    """What to compute, checked when made and immutable.

    ``hop``            samples between frames, 32..512
    ``segment_s``      seconds per segment; ``segment_frames(sr) = round(segment_s * sr / hop)`` must be >= 1
    ``db_threshold``   the level (dB re full scale) a cell has to exceed to count for ``adi`` / ``aei``; ``-inf`` counts every cell that is
                       not zero, ``+inf`` none
    ``band``           the bins of ``aci`` and ``hf`` (``None``: all 257)
    ``bio_band`` ``anthro_band``     of ``bi`` and ``ndsi``
    ``adi_step_hz`` ``adi_max_hz``   the ADI bands ``[j step, (j + 1) step)`` below ``min(adi_max_hz, sr / 2)``
    Bands are checked against the sample rate (none past Nyquist, none without a bin, 1..32 ADI bands) by :meth:`bins`.
    """
    hop: int = 256
    segment_s: float = 60.0
    db_threshold: float = -50.0
    band: Optional[Tuple[float, float]] = None
    bio_band: Tuple[float, float] = (2000.0, 8000.0)
    anthro_band: Tuple[float, float] = (1000.0, 2000.0)
    adi_step_hz: float = 1000.0
    adi_max_hz: float = 10000.0

    def __post_init__(self) -> None:
        if isinstance(self.hop, bool) or not isinstance(self.hop, (int, np.integer)) or not activity.MIN_HOP <= self.hop <= N_FFT:
            raise ValueError(f"hop={self.hop!r}: an integer in {activity.MIN_HOP}..{N_FFT} expected")
        object.__setattr__(self, "hop", int(self.hop))
        s = _number(self.segment_s, "segment_s")
        if s <= 0.0:
            raise ValueError(f"segment_s={s}: a number > 0 expected")
        object.__setattr__(self, "segment_s", s)
        db = self.db_threshold
        if isinstance(db, bool) or not isinstance(db, (int, float, np.integer, np.floating)) or math.isnan(float(db)):
            raise ValueError(f"db_threshold={db!r}: a number expected (-inf and +inf allowed, not NaN)")
        object.__setattr__(self, "db_threshold", float(db))
        if self.band is not None:
            object.__setattr__(self, "band", _band(self.band, "band"))
        object.__setattr__(self, "bio_band", _band(self.bio_band, "bio_band"))
        object.__setattr__(self, "anthro_band", _band(self.anthro_band, "anthro_band"))
        for name in ("adi_step_hz", "adi_max_hz"):
            v = _number(getattr(self, name), name)
            if v <= 0.0:
                raise ValueError(f"{name}={v}: a number > 0 expected")
            object.__setattr__(self, name, v)

    @property
    def threshold(self) -> np.float32:
        """``fl32(P_FS * 10^(db_threshold / 10))``."""
        with np.errstate(over="ignore"):
            return np.float32(np.float64(P_FS) * np.power(np.float64(10.0), np.float64(self.db_threshold) / 10.0))

    def segment_frames(self, sr: int) -> int:
        S = int(round(self.segment_s * int(sr) / self.hop))
        if not 1 <= S <= MAX_SEGMENT_FRAMES:
            raise ValueError(f"segment_s={self.segment_s} at {sr} Hz and hop {self.hop} is {S} frames: 1..{MAX_SEGMENT_FRAMES} expected")
        return S

    def adi_bands(self, sr: int) -> Tuple[Tuple[float, float], ...]:
        J = int(math.floor(min(self.adi_max_hz, int(sr) / 2.0) / self.adi_step_hz))
        if not 1 <= J <= MAX_ADI_BANDS:
            raise ValueError(f"adi_step_hz={self.adi_step_hz}, adi_max_hz={self.adi_max_hz} at {sr} Hz: {J} bands, 1..{MAX_ADI_BANDS} expected")
        return tuple((j * self.adi_step_hz, (j + 1) * self.adi_step_hz) for j in range(J))

    def bins(self, sr: int) -> np.ndarray:
        """The one-element ``INDEX_SPEC_DTYPE`` array the device takes: every band as bins ``k_lo <= k < k_hi`` at sample rate ``sr``."""
        out = np.zeros(1, dtype=INDEX_SPEC_DTYPE)
        out["band"][0] = (0, N_BINS) if self.band is None else activity.band_bins([self.band], sr)[0]
        out["bio"][0] = activity.band_bins([self.bio_band], sr)[0]
        out["anthro"][0] = activity.band_bins([self.anthro_band], sr)[0]
        adi = activity.band_bins(self.adi_bands(sr), sr)
        out["n_adi"][0] = len(adi)
        out["adi"][0, :len(adi)] = adi
        out["bin_khz"][0] = int(sr) / N_FFT / 1000.0
        return out


def segment_plan(n_samples: Sequence[int], hop: int, segment_frames: int, sr: int) -> Dict[str, Any]:
    """The host side of the segments of recordings of ``n_samples`` samples: ``frames`` and ``segments`` per recording,
    ``segment_ranges`` and ``frame_ranges`` (lists of ``(lo, hi)``), and per segment ``recording``, ``first_frame`` (inside its recording),
    ``n_frames``, ``start_s`` and ``end_s``."""
    hop, S = int(hop), int(segment_frames)
    if S < 1:
        raise ValueError(f"segment_frames={S}: at least one frame per segment")
    frames = np.asarray([frame_count(int(n), hop) for n in n_samples], dtype=np.int64)
    segments = (frames + S - 1) // S
    g_end, f_end = np.cumsum(segments), np.cumsum(frames)
    recording = np.repeat(np.arange(len(frames), dtype=np.int32), segments)
    local = np.arange(int(g_end[-1]) if len(g_end) else 0, dtype=np.int64) - np.repeat(g_end - segments, segments)
    first = local * S
    n = np.minimum(S, frames[recording] - first).astype(np.int32)
    return {"frames": frames, "segments": segments, "segment_ranges": [(int(e - c), int(e)) for c, e in zip(segments, g_end)],
            "frame_ranges": [(int(e - c), int(e)) for c, e in zip(frames, f_end)], "recording": recording, "first_frame": first, "n_frames": n,
            "start_s": (first * hop).astype(np.float64) / sr, "end_s": ((first + n - 1) * hop + N_FFT).astype(np.float64) / sr}


class SpectralStats:
    """What :func:`spectral_stats` leaves on the device, with the host segment table.

    ``mean_power`` ``mean_amplitude`` ``abs_diff``   ``[G, 257]`` float32;  ``count_above`` ``[G, 257]`` int32
    ``frame_power``            ``[total_frames]`` float32;  ``frame_ranges[r]`` = the frames ``[f0, f1)`` of recording ``r``
    ``nonfinite_frames``       ``[G]`` int32
    ``segment_ranges[r]``      the segments ``[g0, g1)`` of recording ``r``
    ``recording`` ``n_frames`` ``start_s`` ``end_s``   per segment, host arrays
    ``mean_power`` is the long-term average spectrum: ``10 log10(mean_power / P_FS)`` is dB re full scale.
    """

    def __init__(self, ws: Any, spec: IndexSpec) -> None:
        _capi.require_gpu()
        self.windows, self.spec = ws, spec
        dev = ws.wav.device
        hop, S = spec.hop, spec.segment_frames(ws.sr)
        self.hop, self.segment_frames = hop, S
        self._rec, frames = recording_table(ws, RECORDING_DTYPE, hop)
        plan = segment_plan(self._rec["n_samples"], hop, S, ws.sr)
        segments = plan["segments"]
        runs = (frames // S) * ((S + RUN_FRAMES - 1) // RUN_FRAMES) + (frames % S + RUN_FRAMES - 1) // RUN_FRAMES
        self._rec["first_segment"], self._rec["first_run"] = np.cumsum(segments) - segments, np.cumsum(runs) - runs
        self.total_frames, self.n_segments, self.n_runs = int(frames.sum()), int(segments.sum()), int(runs.sum())
        if max(self.total_frames, self.n_runs) >= 1 << 31:
            raise ValueError(f"{self.total_frames} frames: more than 2^31 - 1 (a longer hop, or fewer recordings per call)")
        self.frame_ranges, self.segment_ranges = plan["frame_ranges"], plan["segment_ranges"]
        self.recording, self.n_frames, self.start_s, self.end_s = plan["recording"], plan["n_frames"], plan["start_s"], plan["end_s"]
        G = self.n_segments
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            self._pinned_rec, self._rec_dev = _to_device(self._rec, dev)
            self._partials_bytes = int(lib().avexhip_soundscape_partials_bytes(self.n_runs))
            self._partials = torch.empty(self._partials_bytes // 4, dtype=torch.float32, device=dev)
            self.frame_power = torch.empty(self.total_frames, dtype=torch.float32, device=dev)
            self.mean_power = torch.empty((G, N_BINS), dtype=torch.float32, device=dev)
            self.mean_amplitude = torch.empty((G, N_BINS), dtype=torch.float32, device=dev)
            self.abs_diff = torch.empty((G, N_BINS), dtype=torch.float32, device=dev)
            self.count_above = torch.empty((G, N_BINS), dtype=torch.int32, device=dev)
            self.nonfinite_frames = torch.empty(G, dtype=torch.int32, device=dev)
            self._frames(stream, _tables_on(dev))
            self._reduce(stream)

    def _ptr(self, t: torch.Tensor) -> Optional[int]:
        return t.data_ptr() if t.numel() else None

    def _table_args(self) -> Tuple[Any, ...]:
        return (self._rec.ctypes.data, self._rec_dev.data_ptr(), len(self._rec), self.hop, self.segment_frames)

    def _frames(self, stream: int, tab: torch.Tensor) -> None:
        ws = self.windows
        rec_host, rec_dev, n_rec, hop, S = self._table_args()
        check(lib().avexhip_soundscape_frames(ws.wav.data_ptr(), ws.wav.numel(), rec_host, rec_dev, n_rec, hop, S, float(self.spec.threshold), tab.data_ptr(),
                                              self.total_frames, self.n_segments, self._ptr(self._partials), self._partials_bytes,
                                              self._ptr(self.frame_power), stream), "soundscape_frames")

    def _reduce(self, stream: int) -> None:
        check(lib().avexhip_soundscape_reduce(*self._table_args(), self.total_frames, self.n_segments, self._ptr(self._partials), self._partials_bytes,
                                              self._ptr(self.mean_power), self._ptr(self.mean_amplitude), self._ptr(self.abs_diff),
                                              self._ptr(self.count_above), self._ptr(self.nonfinite_frames), stream), "soundscape_reduce")


class SoundscapeIndices:
    """What :func:`acoustic_indices` returns: ``stats`` (a :class:`SpectralStats`), ``values`` ``[G, 8]`` float64 on the device in the order
    of :data:`INDEX_NAMES`, and the host segment table (``recording``, ``n_frames``, ``start_s``, ``end_s``, ``segment_ranges``)."""

    def __init__(self, stats: SpectralStats) -> None:
        self.stats, self.spec = stats, stats.spec
        ws = stats.windows
        self._spec_bins = self.spec.bins(ws.sr)
        self.segment_ranges = stats.segment_ranges
        self.recording, self.n_frames, self.start_s, self.end_s = stats.recording, stats.n_frames, stats.start_s, stats.end_s
        dev = ws.wav.device
        with torch.cuda.device(dev):
            self.values = torch.empty((stats.n_segments, len(INDEX_NAMES)), dtype=torch.float64, device=dev)
            self._launch(torch.cuda.current_stream().cuda_stream)

    def _launch(self, stream: int) -> None:
        s = self.stats
        check(lib().avexhip_soundscape_indices(*s._table_args(), s.total_frames, s.n_segments, self._spec_bins.ctypes.data, s._ptr(s.mean_power),
                                               s._ptr(s.mean_amplitude), s._ptr(s.abs_diff), s._ptr(s.count_above), s._ptr(s.nonfinite_frames),
                                               s._ptr(s.frame_power), s._ptr(self.values), stream), "soundscape_indices")

    def column(self, name: str) -> torch.Tensor:
        """One index, ``[G]`` float64 on the device."""
        if name not in INDEX_NAMES:
            raise KeyError(f"{name!r}: one of {INDEX_NAMES}")
        return self.values[:, INDEX_NAMES.index(name)]

    def table(self) -> Dict[str, Any]:
        """The segments on the host (this copies, and waits for the stream): ``recording``, ``name`` where the windows carry names,
        ``start_s``, ``end_s``, ``n_frames`` and one float64 array per index."""
        out: Dict[str, Any] = {"recording": self.recording.copy()}
        names = getattr(self.stats.windows, "names", None)
        if names is not None:
            out["name"] = [names[r] for r in self.recording]
        out.update(start_s=self.start_s.copy(), end_s=self.end_s.copy(), n_frames=self.n_frames.copy())
        host = self.values.cpu().numpy()
        for c, name in enumerate(INDEX_NAMES):
            out[name] = host[:, c].copy()
        return out


def _check(ws: Any, spec: Any) -> None:
    if not isinstance(spec, IndexSpec):
        raise TypeError(f"an IndexSpec expected, not {type(spec).__name__}")
    spec.segment_frames(ws.sr)
    spec.bins(ws.sr)                      # a band the sample rate cannot hold raises here, before anything is launched


def spectral_stats(ws: Any, spec: Optional[IndexSpec] = None) -> SpectralStats:
    """The per-segment spectral statistics of the recordings behind the windows ``ws`` (its window plan plays no part): two launches,
    device tensors, no host synchronisation."""
    spec = IndexSpec() if spec is None else spec
    _check(ws, spec)
    return SpectralStats(ws, spec)


def acoustic_indices(ws: Any, spec: Optional[IndexSpec] = None) -> SoundscapeIndices:
    """The statistics and the eight indices of every segment: three launches, nothing copied back before :meth:`SoundscapeIndices.table`."""
    return SoundscapeIndices(spectral_stats(ws, spec))


def acoustic_indices_of(sources: Sequence[Any], spec: Optional[IndexSpec] = None, *, sr: int = 16000, res_type: Optional[str] = None,
                        device: Any = None) -> SoundscapeIndices:
    """:func:`acoustic_indices` of files, bytes or arrays, read as :func:`avex_amd.recordings.windows` reads them (one window per second:
    the plan is not used)."""
    from . import recordings
    ws = recordings._windows_of(list(sources), 1.0, None, int(sr), "pad", res_type, device, recordings.MAX_RESIDENT_SAMPLES)
    return acoustic_indices(ws, spec)
