"""Band-limited activity gate: which sliding windows hold energy in a frequency band above their recording's own noise floor.

:meth:`avex_amd.recordings.RecordingWindows.select` gates on broadband RMS and peak.  In field recordings those are set by wind, rain, surf
and traffic below 1 kHz: a level gate keeps every windy minute and drops a faint call in a quiet one.  The step that would do better is a
name without a body in the reference (avex/preprocessing/activity_detector.py is an empty file).  Here it is four kernels of
``csrc/activity.hip`` over the resident waveform and the window table of a :class:`~avex_amd.recordings.RecordingWindows`; there is no
CPU fallback.

Semantics (the tests hold them; ``tests/_activity_ref.py`` restates them in NumPy):

* **Frames.**  ``n_fft = 512``; recording ``r`` of ``n_r`` samples has ``F_r = (n_r - 512) // hop + 1`` frames (0 when ``n_r < 512``), frame
  ``f`` the samples ``[f hop, f hop + 512)`` of its recording, no padding.  The frames of all recordings lie back to back.
* **Band energy.**  ``y = x * w`` in fp32 with the periodic Hann table ``w[n] = 0.5 - 0.5 cos(2 pi n / 512)`` (fp64, rounded), ``X = DFT(y)``,
  ``E[b, f]`` the fp32 sum of ``|X[k]|^2`` over ``ceil(lo 512 / sr) <= k < min(ceil(hi 512 / sr), 257)``.  A frame of zeros gives ``+0``, a
  frame with a NaN or an Inf gives NaN, and a frame's energies depend on its recording and the hop alone.
* **Noise floor** per (recording, band): the energy of rank ``floor(p / 100 (F_r - 1))`` among the recording's frames, ordered by bit
  pattern (NaN above ``+inf``); NaN when ``F_r = 0``.
* **Active frame**: ``E > fl32(max(floor, floor_min) * ratio)``, strict, ``ratio = fl32(10^(snr_db / 10))``, ``floor_min = fl32(10^(min_floor_db
  / 10))`` or 0.  With a floor of 0 (digital silence) silent frames are not active and any other frame is.
* **Per window** ``(start, valid)``: its frames are ``ceil(start / hop) .. floor((start + valid - 512) / hop)``; ``n_frames``,
  ``active_frames[w, b]`` and ``max_energy[w, b]`` (NaN if a frame is NaN, ``-inf`` without a frame).
* **Gate**: the RMS / peak conditions of ``RecordingWindows.select`` and ``active_frames[w, b] >= min_active_frames`` in any band
  (``mode="any"``) or in every band (``"all"``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import numpy as np
import torch

from . import _capi
from ._capi import check, lib
from ._frames import N_BINS, N_FFT, _number, _tables_on, _to_device, frame_count, recording_table, tables      # noqa: F401 (names callers find here)

__all__ = ["ActivityGate", "BandActivity", "band_activity", "band_bins", "frame_count", "window_frames", "N_FFT", "MAX_BANDS"]

MAX_BANDS = 8                             # AVEXHIP_ACTIVITY_MAX_BANDS
MIN_HOP = 32                              # AVEXHIP_ACTIVITY_MIN_HOP
BLOCK_FRAMES = 8                          # frames per workgroup of avexhip_activity_frames (avexhip_activity_recording.first_block)
MODES = ("any", "all")                    # AVEXHIP_ACTIVITY_ANY, AVEXHIP_ACTIVITY_ALL
# avexhip_activity_recording, field for field
RECORDING_DTYPE = np.dtype([("base", "<i8"), ("n_samples", "<i8"), ("first_frame", "<i8"), ("first_block", "<i4"), ("floor_rank", "<i4")])


@dataclass(frozen=True)
class ActivityGate:
    """The rule of the gate, checked when made and immutable.

    ``bands``               up to 8 ``(lo_hz, hi_hz)`` pairs, ``0 <= lo < hi``; against the sample rate (no band past Nyquist, none without
                            a bin) they are checked by :meth:`bins`
    ``snr_db``              how far over the floor a frame's band energy has to stand
    ``min_active_frames``   frames a window needs in a band (0: the band condition is off)
    ``mode``                ``"any"`` band or ``"all"`` bands
    ``hop``                 samples between frames, 32..512
    ``floor_percentile``    the floor is that percentile of the recording's frame energies, 0..100
    ``min_floor_db``        a lower bound of the floor in dB (``None``: none), so digital silence does not make every dither frame active
    """
    bands: Tuple[Tuple[float, float], ...]
    snr_db: float = 6.0
    min_active_frames: int = 2
    mode: str = "any"
    hop: int = 256
    floor_percentile: float = 20.0
    min_floor_db: Optional[float] = None

    def __post_init__(self) -> None:
        try:
            bands = tuple((_number(lo, "band"), _number(hi, "band")) for lo, hi in self.bands)
        except TypeError as e:
            raise ValueError(f"bands={self.bands!r}: a sequence of (lo_hz, hi_hz) pairs expected") from e
        if not 1 <= len(bands) <= MAX_BANDS:
            raise ValueError(f"{len(bands)} bands: 1..{MAX_BANDS} expected")
        for lo, hi in bands:
            if not 0.0 <= lo < hi:
                raise ValueError(f"band ({lo}, {hi}): 0 <= lo_hz < hi_hz expected")
        object.__setattr__(self, "bands", bands)
        object.__setattr__(self, "snr_db", _number(self.snr_db, "snr_db"))
        if isinstance(self.min_active_frames, bool) or not isinstance(self.min_active_frames, (int, np.integer)) or self.min_active_frames < 0:
            raise ValueError(f"min_active_frames={self.min_active_frames!r}: an integer >= 0 expected")
        object.__setattr__(self, "min_active_frames", int(self.min_active_frames))
        if self.mode not in MODES:
            raise ValueError(f"mode={self.mode!r}: one of {MODES} expected")
        if isinstance(self.hop, bool) or not isinstance(self.hop, (int, np.integer)) or not MIN_HOP <= self.hop <= N_FFT:
            raise ValueError(f"hop={self.hop!r}: an integer in {MIN_HOP}..{N_FFT} expected")
        object.__setattr__(self, "hop", int(self.hop))
        p = _number(self.floor_percentile, "floor_percentile")
        if not 0.0 <= p <= 100.0:
            raise ValueError(f"floor_percentile={p}: a number in 0..100 expected")
        object.__setattr__(self, "floor_percentile", p)
        if self.min_floor_db is not None:
            object.__setattr__(self, "min_floor_db", _number(self.min_floor_db, "min_floor_db"))

    def bins(self, sr: int) -> np.ndarray:
        """int32 ``[n_bands, 2]``: the bins ``k_lo <= k < k_hi`` of each band at sample rate ``sr``."""
        return band_bins(self.bands, sr)

    @property
    def ratio(self) -> np.float32:
        return np.float32(10.0 ** (self.snr_db / 10.0))

    @property
    def floor_min(self) -> np.float32:
        return np.float32(0.0) if self.min_floor_db is None else np.float32(10.0 ** (self.min_floor_db / 10.0))

    def floor_rank(self, n_frames: int) -> int:
        return int(math.floor(self.floor_percentile / 100.0 * (n_frames - 1))) if n_frames > 0 else 0


def band_bins(bands, sr: int) -> np.ndarray:
    """``k_lo = ceil(lo 512 / sr)``, ``k_hi = min(ceil(hi 512 / sr), 257)`` per band; a band past Nyquist or without a bin raises."""
    sr = int(sr)
    if sr <= 0:
        raise ValueError(f"sr={sr}")
    out = np.zeros((len(bands), 2), dtype=np.int32)
    for b, (lo, hi) in enumerate(bands):
        k_lo, k_hi = math.ceil(lo * N_FFT / sr), min(math.ceil(hi * N_FFT / sr), N_BINS)
        if not 0 <= k_lo < k_hi:            # between two bins, or past the Nyquist frequency
            raise ValueError(f"band ({lo}, {hi}) Hz holds no bin of a {N_FFT}-point transform at {sr} Hz (Nyquist {sr / 2.0} Hz)")
        out[b] = (k_lo, k_hi)
    return out


def window_frames(start: int, valid: int, hop: int) -> Tuple[int, int]:
    """``(f_lo, n_frames)`` of a window: the frames that lie wholly inside ``[start, start + valid)``."""
    f_lo = -(-int(start) // int(hop))
    end = int(start) + int(valid) - N_FFT
    f_hi = -1 if end < 0 else end // int(hop)
    return f_lo, max(0, f_hi - f_lo + 1)


class BandActivity:
    """What :func:`band_activity` leaves on the device.

    ``frame_energy``       ``[n_bands, total_frames]`` float32;  ``frame_ranges[r]`` = the frames ``[f0, f1)`` of recording ``r``
    ``floor``              ``[n_recordings, n_bands]`` float32;  ``nonfinite_frames`` ``[n_recordings]`` int32
    ``n_frames``           ``[n_windows]`` int32;  ``active_frames`` ``[n_windows, n_bands]`` int32;  ``max_energy`` the same shape, float32
    ``select(...)``        the kept list, in the format of :meth:`avex_amd.recordings.RecordingWindows.select`
    """

    def __init__(self, ws: Any, gate: ActivityGate) -> None:
        _capi.require_gpu()
        self.windows, self.gate = ws, gate
        self.bins = gate.bins(ws.sr)
        dev = ws.wav.device
        n_rec, n_bands, n_win, hop = len(ws.ranges), len(self.bins), ws.n_windows, gate.hop
        self._rec, counts = recording_table(ws, RECORDING_DTYPE, hop)
        blocks = (counts + BLOCK_FRAMES - 1) // BLOCK_FRAMES
        self._rec["first_block"], self._rec["floor_rank"] = np.cumsum(blocks) - blocks, [gate.floor_rank(int(c)) for c in counts]
        self.total_frames = int(counts.sum())
        self.frame_ranges: List[Tuple[int, int]] = [(int(f), int(f + c)) for f, c in zip(self._rec["first_frame"], counts)]
        self._win_rec = np.ascontiguousarray(ws.recording, dtype=np.int32)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            self._pinned_rec, self._rec_dev = _to_device(self._rec, dev)
            self._pinned_win_rec, self._win_rec_dev = _to_device(self._win_rec, dev)
            self.frame_energy = torch.empty((n_bands, self.total_frames), dtype=torch.float32, device=dev)
            self.floor = torch.empty((n_rec, n_bands), dtype=torch.float32, device=dev)
            self.nonfinite_frames = torch.empty(n_rec, dtype=torch.int32, device=dev)
            self.n_frames = torch.empty(n_win, dtype=torch.int32, device=dev)
            self.active_frames = torch.empty((n_win, n_bands), dtype=torch.int32, device=dev)
            self.max_energy = torch.empty((n_win, n_bands), dtype=torch.float32, device=dev)
            energy_ptr = self.frame_energy.data_ptr() if self.total_frames else None
            rec_host, rec_dev = self._rec.ctypes.data, self._rec_dev.data_ptr()
            check(lib().avexhip_activity_frames(ws.wav.data_ptr(), ws.wav.numel(), rec_host, rec_dev, n_rec, hop, self.bins.ctypes.data, n_bands,
                                                _tables_on(dev).data_ptr(), self.total_frames, energy_ptr, stream), "activity_frames")
            check(lib().avexhip_activity_floor(energy_ptr, self.total_frames, rec_host, rec_dev, n_rec, hop, n_bands, self.floor.data_ptr(),
                                               self.nonfinite_frames.data_ptr(), stream), "activity_floor")
            check(lib().avexhip_activity_count(ws._table.ctypes.data, ws._table_dev.data_ptr(), self._win_rec.ctypes.data, self._win_rec_dev.data_ptr(), n_win,
                                               rec_host, rec_dev, n_rec, hop, energy_ptr, self.total_frames, self.floor.data_ptr(), n_bands,
                                               float(gate.floor_min), float(gate.ratio), self.n_frames.data_ptr(), self.active_frames.data_ptr(),
                                               self.max_energy.data_ptr(), stream), "activity_count")

    def select(self, min_rms_db: Optional[float] = None, min_peak_db: Optional[float] = None) -> torch.Tensor:
        """int32 ``[n_windows + 1]`` on the device, no copy to the host: the windows that pass the level thresholds (``None``: off) and the
        band condition, in increasing order in ``[:k]``, the count ``k`` in ``[n_windows]``."""
        ws, gate = self.windows, self.gate
        thr_e = -math.inf if min_rms_db is None else 10.0 ** (float(min_rms_db) / 10.0)
        thr_p = -math.inf if min_peak_db is None else 10.0 ** (float(min_peak_db) / 20.0)
        n = ws.n_windows
        with torch.cuda.device(ws.wav.device):
            out = torch.empty(n + 1, dtype=torch.int32, device=ws.wav.device)
            check(lib().avexhip_activity_select(ws._table_dev.data_ptr(), ws.energy.data_ptr(), ws.peak.data_ptr(), self.active_frames.data_ptr(), n,
                                                len(self.bins), gate.min_active_frames, MODES.index(gate.mode), thr_e, thr_p, out.data_ptr(),
                                                out.data_ptr() + 4 * n, torch.cuda.current_stream().cuda_stream), "activity_select")
        return out


def band_activity(ws: Any, gate: ActivityGate) -> BandActivity:
    """Frame band energies, noise floors and per-window active-frame counts of the windows ``ws`` under ``gate``: three launches, device
    tensors, no host synchronisation."""
    if not isinstance(gate, ActivityGate):
        raise TypeError(f"an ActivityGate expected, not {type(gate).__name__}")
    return BandActivity(ws, gate)
