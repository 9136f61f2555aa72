"""Event measurements: the time and frequency extent of each event -- what a selection table carries beside the class.

:func:`avex_amd.detection.decode_events` says "class c, windows 25..34, peak 0.93": its bounds are window edges and it has no frequency
extent.  :func:`measure_events` looks at the samples behind each event and reports where its energy lies: the band that holds
``energy_fraction`` of it, its centre and peak frequency, and the stretch of frames that holds the same fraction in time, optionally
after a noise spectrum (:func:`noise_spectrum`) is taken off.  :func:`write_raven` writes events with those bounds as a Raven selection
table that :meth:`avex_amd.annotations.Annotations.from_raven` reads back.  Two kernels of ``csrc/measure.hip``; no CPU fallback.

Semantics (the tests hold them; ``tests/_measure_ref.py`` restates them in NumPy):

* **Boxes.**  An event is a box on one recording ``r`` of a :class:`~avex_amd.recordings.RecordingWindows` ``ws``: the samples
  ``[s0, s1)`` counted from the recording's first, and the bins ``[lo, hi)``, ``0 <= lo < hi <= 257``.  For an event of ``decode_events``,
  ``s0 = ws.starts[first]``, ``s1 = ws.starts[last] + ws.valids[last]`` and ``r = sequence``.  The band is ``MeasureSpec.band``: ``None`` is
  all 257 bins, one ``(lo_hz, hi_hz)`` serves every class, a sequence of ``C`` pairs gives one per class; Hz become bins by
  :func:`avex_amd.activity.band_bins`.
* **Frames** as in :mod:`avex_amd.soundscape`, on the recording's own grid: 512 samples every ``hop`` (32..512), the fp32 periodic Hann
  table of ``activity.tables()``, one frame per transform: ``P[f, k]`` is the same function of the frame's 512 samples as there (``+0`` in
  every bin for a frame of zeros, NaN in every bin for a frame with a NaN or an Inf).  The event's frames are those wholly inside
  ``[s0, s1)``: ``f0 = ceil(s0 / hop)``, ``f1 = min((s1 - 512) // hop + 1, F_r)`` when ``s1 >= 512`` else 0, ``n = max(f1 - f0, 0)``.
* **Statistics** (fp32).  ``spectrum[e, k]`` = the sum of ``P[f, k]`` over the event's frames for ``lo <= k < hi``, ``+0`` outside the band:
  runs of 64 frames counted from ``f0``, frame order inside a run, the runs added in run order (the order of a soundscape segment).
  ``envelope[o_e + t]`` = the band energy of frame ``f0 + t``, formed as soundscape's ``frame_power`` (bins outside the band add ``+0``),
  ``o_e = frame_offsets[e]``.  ``nonfinite[e]`` counts the event's non-finite frames; with one, ``spectrum[e]`` is NaN in every band bin and
  ``envelope`` keeps the per-frame values.
* **Measurements**, fp64 on the device from those statistics.  With ``noise_power [R, 257]`` (fp32: mean power per frame and bin),
  ``S'[k] = max(spectrum[k] - n noise[r, k], 0)`` and ``e'[t] = max(envelope[t] - sum_band noise[r, k], 0)`` (the noise sum in bin order);
  without, ``S' = spectrum`` and ``e' = envelope``.  ``energy_fraction = p`` gives the levels ``q_lo = (1 - p) / 2``, ``q_c = 0.5``,
  ``q_hi = 1 - q_lo``; the quantile index of level ``q`` over ``v`` is the smallest ``i`` with ``cumsum(v)[i] >= q sum(v)``.

  ``n_frames`` ``nonfinite``                       int32
  ``energy``                                       ``sum S'``
  ``low_bin`` ``centre_bin`` ``high_bin``          the quantile bins of ``S'``;  ``peak_bin`` the lowest bin attaining ``max S'``
  ``low_frame`` ``centre_frame`` ``high_frame``    the quantile frames of ``e'``, numbered on the recording's grid;  ``peak_frame``
  ``snr_db``                                       ``10 log10(sum S' / (n sum_band noise))``; NaN without noise or when that is 0

  and, derived by torch on the device: ``low_hz centre_hz high_hz peak_hz = bin sr / 512``, ``bandwidth_hz = high_hz - low_hz + sr / 512``,
  ``begin_s = low_frame hop / sr`` (from the recording's start), ``end_s = (high_frame hop + 512) / sr``, ``centre_s`` / ``peak_s`` =
  ``(frame hop + 256) / sr``, ``duration_s = end_s - begin_s``.

  An event with ``n = 0`` (shorter than a frame) or a non-finite frame has ``-1`` in the eight index columns and NaN in every float
  column; with ``sum S' = 0`` the bin columns are ``-1`` (their Hz NaN), with ``sum e' = 0`` the frame columns (their seconds NaN).  A
  padded row of ``decode_events`` (``first == -1``) has ``n_frames = -1``, ``-1`` and NaN, a zero row of ``spectrum`` and no envelope; it is
  never launched.

An event's numbers depend on its recording's samples, its box, ``hop``, ``p`` and its noise row alone: the same bits in any company, in
any order of the events (which may overlap and repeat) and on every run.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi, activity
from ._capi import check, lib
from ._frames import N_BINS, N_FFT, _number, _tables_on, _to_device, frame_count

__all__ = ["MeasureSpec", "Measurements", "event_frames", "measure_boxes", "measure_events", "noise_spectrum", "write_raven", "INT_COLUMNS", "FLOAT_COLUMNS"]

RUN_FRAMES = 64                           # AVEXHIP_MEASURE_RUN_FRAMES
MAX_EVENT_FRAMES = 1 << 24                # AVEXHIP_MEASURE_MAX_EVENT_FRAMES
# avexhip_measure_event and avexhip_measure_result, field for field
EVENT_DTYPE = np.dtype([("base", "<i8"), ("n_samples", "<i8"), ("s0", "<i8"), ("s1", "<i8"), ("env_offset", "<i8"), ("n_frames", "<i4"), ("first_run", "<i4"),
                        ("lo", "<i4"), ("hi", "<i4"), ("recording", "<i4"), ("reserved", "<i4")])
INT_COLUMNS = ("n_frames", "nonfinite", "low_bin", "centre_bin", "high_bin", "peak_bin", "low_frame", "centre_frame", "high_frame", "peak_frame")
FLOAT_COLUMNS = ("energy", "snr_db")
RESULT_DTYPE = np.dtype([(name, "<u8") for name in ("n_frames", "nonfinite", "energy", "low_bin", "centre_bin", "high_bin", "peak_bin", "low_frame",
                                                      "centre_frame", "high_frame", "peak_frame", "snr_db")])
RAVEN_COLUMNS = ("Selection", "View", "Channel", "Begin Time (s)", "End Time (s)", "Low Freq (Hz)", "High Freq (Hz)")


def _pair(x: Any, what: str) -> Tuple[float, float]:
    try:
        lo, hi = x
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}={x!r}: a (lo_hz, hi_hz) pair expected") from e
    lo, hi = _number(lo, what), _number(hi, what)
    if not 0.0 <= lo < hi:
        raise ValueError(f"{what} ({lo}, {hi}): 0 <= lo_hz < hi_hz expected")
    return lo, hi


def _is_number(x: Any) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


@dataclass(frozen=True)
class MeasureSpec:
    """What to measure, checked when made and immutable.

    ``hop``               samples between frames, 32..512
    ``band``              ``None`` (all 257 bins), one ``(lo_hz, hi_hz)`` for every class, or a sequence of such pairs, one per class
    ``energy_fraction``   ``p`` in (0, 1): the share of the energy between the low and the high bound, in frequency and in time
    Bands are checked against the sample rate (none past Nyquist, none without a bin) by :meth:`bins`.
    """
    hop: int = 128
    band: Optional[Any] = None
    energy_fraction: float = 0.9

    def __post_init__(self) -> None:
        if isinstance(self.hop, bool) or not isinstance(self.hop, (int, np.integer)) or not activity.MIN_HOP <= self.hop <= N_FFT:
            raise ValueError(f"hop={self.hop!r}: an integer in {activity.MIN_HOP}..{N_FFT} expected")
        object.__setattr__(self, "hop", int(self.hop))
        p = _number(self.energy_fraction, "energy_fraction")
        if not 0.0 < p < 1.0:
            raise ValueError(f"energy_fraction={p}: a number in (0, 1) expected")
        object.__setattr__(self, "energy_fraction", p)
        b = self.band
        if b is not None:
            if isinstance(b, (str, bytes)) or _is_number(b) or isinstance(b, bool):
                raise ValueError(f"band={b!r}: None, a (lo_hz, hi_hz) pair or a sequence of pairs expected")
            try:
                items = list(b)
            except TypeError as e:
                raise ValueError(f"band={b!r}: None, a (lo_hz, hi_hz) pair or a sequence of pairs expected") from e
            if len(items) == 2 and all(_is_number(v) or isinstance(v, bool) for v in items):
                b = _pair(items, "band")
            else:
                if len(items) == 0:
                    raise ValueError("band=(): at least one (lo_hz, hi_hz) pair expected")
                b = tuple(_pair(v, f"band[{c}]") for c, v in enumerate(items))
            object.__setattr__(self, "band", b)

    @property
    def per_class(self) -> bool:
        return self.band is not None and isinstance(self.band[0], tuple)

    @property
    def levels(self) -> Tuple[float, float, float]:
        """``(q_lo, q_c, q_hi)`` in float64."""
        q_lo = (1.0 - self.energy_fraction) / 2.0
        return q_lo, 0.5, 1.0 - q_lo

    def bins(self, sr: int) -> np.ndarray:
        """``[1, 2]`` (one band for every class) or ``[C, 2]`` int32 bins ``k_lo <= k < k_hi`` at sample rate ``sr``."""
        if self.band is None:
            return np.asarray([[0, N_BINS]], dtype=np.int32)
        return activity.band_bins(list(self.band) if self.per_class else [self.band], sr)


def event_frames(start: Any, end: Any, hop: int, n_samples: Any) -> Tuple[np.ndarray, np.ndarray]:
    """``(f0, n)`` (int64 arrays): the frames of a recording of ``n_samples`` samples that lie wholly inside ``[start, end)``."""
    s0, s1, ns = (np.asarray(v, dtype=np.int64) for v in (start, end, n_samples))
    hop = int(hop)
    F = np.where(ns < N_FFT, 0, (ns - N_FFT) // hop + 1)
    f0 = -((-s0) // hop)
    f1 = np.minimum(np.where(s1 >= N_FFT, (s1 - N_FFT) // hop + 1, 0), F)
    f0, f1 = np.broadcast_arrays(f0, f1)
    return f0.astype(np.int64), np.maximum(f1 - f0, 0).astype(np.int64)


def _host_ints(x: Any, what: str) -> np.ndarray:
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{what}: a 1-d integer array expected")
    return a.astype(np.int64)


def _recordings_of(ws: Any) -> Tuple[np.ndarray, np.ndarray]:
    first = np.asarray([w0 for w0, _ in ws.ranges], dtype=np.int64)
    return ws._table["base"][first].astype(np.int64), ws._table["n_samples"][first].astype(np.int64)


def _filled(shape: Any, dtype: torch.dtype, dev: torch.device) -> torch.Tensor:
    return torch.full(shape, -1 if dtype == torch.int32 else math.nan, dtype=dtype, device=dev)


class Measurements(dict):
    """What :func:`measure_boxes` returns: a dict of device tensors, one row per box (``envelope`` one value per frame,
    ``frame_offsets [E + 1]``), with the ``sr`` and ``hop`` they were made at as attributes."""
    sr: int
    hop: int


def measure_boxes(ws: Any, recording: Any, start_sample: Any, end_sample: Any, spec: Optional[MeasureSpec] = None, *, class_id: Any = None,
                  noise_power: Optional[torch.Tensor] = None, bins: Any = None) -> "Measurements":
    """The measurements of the boxes ``[start_sample, end_sample)`` (counted from the recording's first sample) of the recordings
    ``recording`` behind the windows ``ws`` (its window plan plays no part).  The three arrays are host integers (``[E]``); a row with
    ``recording == -1`` is a padded row.  ``class_id [E]`` picks each box's band when ``spec.band`` holds one per class.  ``bins [E, 2]``
    (host integers): each box's own bins ``lo <= k < hi``, ``0 <= lo < hi <= 257``, in place of ``spec.band`` and ``class_id`` (a padded
    row's pair is not read) -- the boxes of :meth:`avex_amd.regions.Regions.boxes`.
    ``noise_power [R, 257]``: a device tensor, e.g. :func:`noise_spectrum`.  Two launches, device tensors, no host synchronisation.
    See the module docstring for the columns; ``first_frame [E]`` (``f0``), ``recording`` and the box's own span ``box_begin_s`` /
    ``box_end_s`` come with them."""
    spec = MeasureSpec() if spec is None else spec
    if not isinstance(spec, MeasureSpec):
        raise TypeError(f"a MeasureSpec expected, not {type(spec).__name__}")
    rec, s0, s1 = _host_ints(recording, "recording"), _host_ints(start_sample, "start_sample"), _host_ints(end_sample, "end_sample")
    E = len(rec)
    if len(s0) != E or len(s1) != E:
        raise ValueError(f"{E} recordings, {len(s0)} starts and {len(s1)} ends: one of each per box expected")
    sr, hop = int(ws.sr), spec.hop
    bands = spec.bins(sr)                                        # a band the sample rate cannot hold raises here, before anything is launched
    base, n_samples = _recordings_of(ws)
    R = len(base)
    real = rec >= 0
    idx = np.flatnonzero(real)
    if (rec < -1).any() or (rec >= R).any():
        raise ValueError(f"recording outside -1..{R - 1}")
    r_, a_, b_ = rec[idx], s0[idx], s1[idx]
    if ((a_ < 0) | (b_ < a_) | (b_ > n_samples[r_])).any():
        e = int(idx[np.argmax((a_ < 0) | (b_ < a_) | (b_ > n_samples[r_]))])
        raise ValueError(f"box {e}: samples {int(s0[e])}..{int(s1[e])} outside recording {int(rec[e])} of {int(n_samples[rec[e]])} samples")
    if bins is not None:
        own = np.asarray(bins.detach().cpu() if isinstance(bins, torch.Tensor) else bins)
        if own.shape != (E, 2) or (own.size and own.dtype.kind not in "iu"):
            raise ValueError(f"bins: an integer [{E}, 2] array expected")
        lo_hi = own.astype(np.int64)[idx]
        if ((lo_hi[:, 0] < 0) | (lo_hi[:, 0] >= lo_hi[:, 1]) | (lo_hi[:, 1] > N_BINS)).any():
            e = int(idx[np.argmax((lo_hi[:, 0] < 0) | (lo_hi[:, 0] >= lo_hi[:, 1]) | (lo_hi[:, 1] > N_BINS))])
            raise ValueError(f"box {e}: bins {int(own[e, 0])}..{int(own[e, 1])} outside 0 <= lo < hi <= {N_BINS}")
    elif spec.per_class:
        if class_id is None:
            raise ValueError("spec.band holds one band per class: class_id expected")
        cls = _host_ints(class_id, "class_id")
        if len(cls) != E:
            raise ValueError(f"{len(cls)} class ids for {E} boxes")
        c_ = cls[idx]
        if ((c_ < 0) | (c_ >= len(bands))).any():
            raise ValueError(f"class_id outside 0..{len(bands) - 1}, the bands of spec.band")
        lo_hi = bands[c_]
    else:
        lo_hi = np.broadcast_to(bands[0], (len(idx), 2))
    f0_, n_ = event_frames(a_, b_, hop, n_samples[r_])
    if len(n_) and int(n_.max()) > MAX_EVENT_FRAMES:
        raise ValueError(f"a box of {int(n_.max())} frames: more than 2^24 (a longer hop, or shorter boxes)")
    runs = (n_ + RUN_FRAMES - 1) // RUN_FRAMES
    total_frames, total_runs, Ev = int(n_.sum()), int(runs.sum()), len(idx)
    if max(total_frames, total_runs) >= 1 << 31:
        raise ValueError(f"{total_frames} frames: more than 2^31 - 1 (a longer hop, or fewer boxes per call)")
    table = np.zeros(Ev, dtype=EVENT_DTYPE)
    table["base"], table["n_samples"], table["s0"], table["s1"] = base[r_], n_samples[r_], a_, b_
    table["env_offset"], table["n_frames"], table["first_run"] = np.cumsum(n_) - n_, n_, np.cumsum(runs) - runs
    table["lo"], table["hi"], table["recording"] = lo_hi[:, 0], lo_hi[:, 1], r_
    n_all, f0_all = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    n_all[idx], f0_all[idx] = n_, f0_
    offsets = np.zeros(E + 1, dtype=np.int64)
    np.cumsum(n_all, out=offsets[1:])

    _capi.require_gpu()
    dev = ws.wav.device
    noise = None
    if noise_power is not None:
        if not isinstance(noise_power, torch.Tensor) or tuple(noise_power.shape) != (R, N_BINS) or not noise_power.is_floating_point():
            raise ValueError(f"noise_power: a float [{R}, {N_BINS}] tensor expected")
        noise = noise_power.to(device=dev, dtype=torch.float32).contiguous()
    q_lo, q_c, q_hi = spec.levels
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        cols = {name: torch.empty(Ev, dtype=torch.int32, device=dev) for name in INT_COLUMNS}
        cols.update({name: torch.empty(Ev, dtype=torch.float64, device=dev) for name in FLOAT_COLUMNS})
        spectrum = torch.empty((Ev, N_BINS), dtype=torch.float32, device=dev)
        envelope = torch.empty(total_frames, dtype=torch.float32, device=dev)
        keep = []                                                # what the stream still reads when this returns
        if Ev:
            pinned, table_dev = _to_device(table, dev)
            pbytes = int(lib().avexhip_measure_partials_bytes(total_runs))
            partials = torch.empty(pbytes // 4, dtype=torch.float32, device=dev)
            res = np.zeros(1, dtype=RESULT_DTYPE)
            for name in RESULT_DTYPE.names:
                res[name][0] = cols[name].data_ptr()
            ptr = lambda t: t.data_ptr() if t.numel() else None
            tab, compact = _tables_on(dev), spectrum

            def frames(stream: int) -> None:
                check(lib().avexhip_measure_frames(ws.wav.data_ptr(), ws.wav.numel(), table.ctypes.data, table_dev.data_ptr(), Ev, hop, tab.data_ptr(), total_frames,
                                                   total_runs, ptr(partials), pbytes, ptr(envelope), stream), "measure_frames")

            def reduce(stream: int) -> None:
                check(lib().avexhip_measure_reduce(table.ctypes.data, table_dev.data_ptr(), Ev, hop, total_frames, total_runs, ptr(partials), pbytes, ptr(envelope),
                                                   noise.data_ptr() if noise is not None else None, R, q_lo, q_c, q_hi, compact.data_ptr(), res.ctypes.data,
                                                   stream), "measure_reduce")

            frames(stream)
            reduce(stream)
            keep = [pinned, table_dev, partials, noise, frames, reduce]     # the two launches again, for scripts/measure_bench.py
        if Ev != E:                                              # padded rows: -1 / NaN, a zero row of spectrum
            at = torch.from_numpy(idx).to(dev)
            full = {name: _filled((E,), t.dtype, dev).index_copy_(0, at, t) for name, t in cols.items()}
            spectrum = torch.zeros((E, N_BINS), dtype=torch.float32, device=dev).index_copy_(0, at, spectrum)
            cols = full
        out = Measurements(cols)
        nan = torch.full((), math.nan, dtype=torch.float64, device=dev)

        def where(col: str, value: torch.Tensor) -> torch.Tensor:
            return torch.where(out[col] >= 0, value, nan)

        for name in ("low", "centre", "high", "peak"):
            out[f"{name}_hz"] = where(f"{name}_bin", out[f"{name}_bin"].to(torch.float64) * sr / N_FFT)
        out["bandwidth_hz"] = out["high_hz"] - out["low_hz"] + sr / N_FFT
        out["begin_s"] = where("low_frame", (out["low_frame"].to(torch.int64) * hop).to(torch.float64) / sr)
        out["end_s"] = where("high_frame", (out["high_frame"].to(torch.int64) * hop + N_FFT).to(torch.float64) / sr)
        out["centre_s"] = where("centre_frame", (out["centre_frame"].to(torch.int64) * hop + N_FFT // 2).to(torch.float64) / sr)
        out["peak_s"] = where("peak_frame", (out["peak_frame"].to(torch.int64) * hop + N_FFT // 2).to(torch.float64) / sr)
        out["duration_s"] = out["end_s"] - out["begin_s"]
        out.update(spectrum=spectrum, envelope=envelope, frame_offsets=torch.from_numpy(offsets).to(dev), first_frame=torch.from_numpy(f0_all).to(dev),
                   recording=torch.from_numpy(rec.astype(np.int32)).to(dev), box_begin_s=torch.from_numpy(np.where(real, s0 / sr, np.nan)).to(dev),
                   box_end_s=torch.from_numpy(np.where(real, s1 / sr, np.nan)).to(dev))
        out.sr, out.hop, out._keep = sr, hop, keep
    return out


def measure_events(events: Dict[str, Any], ws: Any, spec: Optional[MeasureSpec] = None, *, noise_power: Optional[torch.Tensor] = None) -> Dict[str, Any]:
    """The measurements of the events of :func:`avex_amd.detection.decode_events` / ``detect_events`` over the windows ``ws`` they were
    decoded with, row for row (padded rows, ``first == -1``, give ``-1`` / NaN).  ``sequence``, ``class_id``, ``first`` and ``last`` are
    read to the host once -- the call's one synchronisation, needed to plan the runs; everything returned stays on the device."""
    cols = torch.stack([events[k].to(torch.int32) for k in ("sequence", "class_id", "first", "last")]).cpu().numpy().astype(np.int64)
    seq, cls, first, last = cols
    real = first >= 0
    if (first[real] >= ws.n_windows).any() or (last[real] >= ws.n_windows).any() or (last[real] < first[real]).any():
        raise ValueError(f"events outside the {ws.n_windows} windows")
    top = max(ws.n_windows - 1, 0)
    f, l = np.clip(first, 0, top), np.clip(last, 0, top)
    if ws.n_windows and (ws.recording[f[real]] != seq[real]).any():
        raise ValueError("an event's windows do not belong to its sequence: other windows than the events were decoded with")
    starts, valids = np.asarray(ws.starts, dtype=np.int64), np.asarray(ws.valids, dtype=np.int64)
    s0 = np.where(real, starts[f], 0) if ws.n_windows else np.zeros_like(first)
    s1 = np.where(real, starts[l] + valids[l], 0) if ws.n_windows else np.zeros_like(first)
    return measure_boxes(ws, np.where(real, seq, -1), s0, s1, spec, class_id=np.where(real, cls, 0), noise_power=noise_power)


def noise_spectrum(stats: Any) -> torch.Tensor:
    """``[R, 257]`` float32 on the device, for a :class:`avex_amd.soundscape.SpectralStats`: per recording and bin the minimum of
    ``mean_power`` over that recording's segments that are full (``n_frames == S``) and hold no non-finite frame; NaN where there is
    none.  torch only."""
    dev = stats.mean_power.device
    R = len(stats.segment_ranges)
    out = torch.full((R, N_BINS), math.nan, dtype=torch.float32, device=dev)
    if stats.n_segments == 0:
        return out
    full = torch.from_numpy(np.asarray(stats.n_frames) == stats.segment_frames).to(dev) & (stats.nonfinite_frames == 0)
    power = torch.where(full[:, None], stats.mean_power, torch.full((), math.inf, dtype=torch.float32, device=dev))
    rec = torch.from_numpy(np.asarray(stats.recording, dtype=np.int64)).to(dev)
    low = torch.full((R, N_BINS), math.inf, dtype=torch.float32, device=dev).scatter_reduce(0, rec[:, None].expand(-1, N_BINS), power, "amin")
    return torch.where(torch.isinf(low), out, low)


def _host(x: Any) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def write_raven(path: Any, events: Dict[str, Any], measurements: Optional[Dict[str, Any]] = None, *, recording: int, class_names: Optional[Sequence[str]] = None,
                class_column: str = "Species", sr: Optional[int] = None) -> int:
    """One tab-separated Raven selection table for recording ``recording``: ``Selection``, ``View``, ``Channel``, ``Begin Time (s)``,
    ``End Time (s)``, ``Low Freq (Hz)``, ``High Freq (Hz)``, ``class_column`` and ``Score`` (the event's ``peak``).  Begin and end come from
    ``measurements`` where its frame columns are ``>= 0`` and the frequencies where its bin columns are, else from the event's window span
    (``start_s`` / ``end_s``: events decoded with ``windows=``) and 0 .. ``sr / 2`` (``sr``: that of the measurements, else 16000).  Times are
    written with ``repr`` and read back exactly.  Host tensors or NumPy arrays; padded rows are skipped.  Returns the rows written."""
    ev = {k: _host(events[k]) for k in ("class_id", "first", "peak", "start_s", "end_s") if k in events}
    rec = _host(events["recording"] if "recording" in events else events["sequence"])
    for k in ("class_id", "first", "peak"):
        if k not in ev:
            raise ValueError(f"events without {k!r}: the dict of decode_events expected")
    m = None
    if measurements is not None:
        m = {k: _host(measurements[k]) for k in ("low_frame", "high_frame", "low_bin", "high_bin", "begin_s", "end_s", "low_hz", "high_hz")}
        if len(m["low_frame"]) != len(rec):
            raise ValueError(f"{len(m['low_frame'])} measurements for {len(rec)} events")
        sr = getattr(measurements, "sr", None) if sr is None else sr
    nyquist = (16000 if sr is None else int(sr)) / 2.0
    rows = 0
    with open(os.fspath(path), "w", newline="", encoding="utf-8") as f:
        f.write("\t".join(RAVEN_COLUMNS + (class_column, "Score")) + "\n")
        for e in range(len(rec)):
            if int(ev["first"][e]) < 0 or int(rec[e]) != int(recording):
                continue
            low, high = 0.0, nyquist
            if m is not None and int(m["low_frame"][e]) >= 0 and int(m["high_frame"][e]) >= 0:
                begin, end = float(m["begin_s"][e]), float(m["end_s"][e])
            elif "start_s" in ev and "end_s" in ev:
                begin, end = float(ev["start_s"][e]), float(ev["end_s"][e])
            else:
                raise ValueError(f"event {e} has no measured bounds and the events carry no start_s / end_s (decode them with windows=)")
            if m is not None and int(m["low_bin"][e]) >= 0 and int(m["high_bin"][e]) >= 0:
                low, high = float(m["low_hz"][e]), float(m["high_hz"][e])
            c = int(ev["class_id"][e])
            name = str(class_names[c]) if class_names is not None else str(c)
            rows += 1
            f.write("\t".join([str(rows), "Spectrogram 1", "1", repr(begin), repr(end), repr(low), repr(high), name, repr(float(ev["peak"][e]))]) + "\n")
    return rows
