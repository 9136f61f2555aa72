"""Sound-event regions: model-free segmentation of unlabelled recordings -- one time-frequency box per sound.

Every other detector of the package needs something to exist first: a trained probe, labelled examples, boxes from somebody else.
:func:`find_regions` needs a recording alone.  It thresholds the spectrogram against the recording's own noise spectrum
(:func:`avex_amd.measurements.noise_spectrum`), joins the cells that stand out into connected regions and returns one box per region --
the band-limited energy detector of Raven and every "blob" detector.  :func:`label_cells` does the joining for a mask from anywhere.
The kernels of ``csrc/regions.hip``; no CPU fallback.  The ``[frames, 257]`` spectrogram is never stored: 9 words of cell bits per frame
are, one integer per frame and nine per set cell.

Semantics (the tests hold them bit for bit; ``tests/_regions_ref.py`` restates them in NumPy):

* **Frames and power** as in :mod:`avex_amd.soundscape`, on the recording's own grid: 512 samples every ``hop`` (32..512), the fp32
  periodic Hann table of ``activity.tables()``, one frame per transform, ``P[f, k]`` for ``k = 0..256`` -- ``+0`` in every bin for a frame
  of zeros, NaN in every bin for a frame with a NaN or an Inf.
* **Threshold** ``thr [R, 257]`` float32, made by torch on the device before the launch:
  ``thr[r, k] = maximum(noise_power[r, k] * ratio32, floor32)`` with ``ratio32 = float32(10 ** (snr_db / 10))`` and
  ``floor32 = float32(16384 * 10 ** (min_db / 10))`` (soundscape's ``threshold`` convention; ``min_db=None``: 0).  Without
  ``noise_power`` the threshold is ``floor32`` everywhere and ``min_db`` must be given.  ``torch.maximum`` propagates a NaN: a NaN noise
  row (a recording with no full finite segment) gives a NaN threshold and therefore no cells in that recording.
* **Cells.**  Cell ``(f, k)`` is set iff ``lo <= k < hi`` and ``P[f, k] > thr[r, k]``: one strict fp32 compare, false for a NaN.  The band
  is ``spec.band`` in Hz through :func:`avex_amd.activity.band_bins` (``None``: all 257 bins).  ``nonfinite_frames [R]`` counts each
  recording's NaN frames.  The mask is an output: ``cells [total_frames, 9]`` int32, bit ``k % 32`` of word ``k // 32`` is cell ``(f, k)``;
  a recording's frames lie back to back in recording order (``frame_offsets [R + 1]``).
* **Neighbours.**  ``reach = (rt, rk)``, ``0 <= rt <= 4``, ``0 <= rk <= 8``, default ``(1, 1)`` (8-connectivity): two set cells of one
  recording are neighbours when ``|df| <= rt`` and ``|dk| <= rk``; a larger reach bridges the gaps a closing would.  Regions are the
  connected components.  A region never crosses into the next recording, and bin 256 of a frame is no neighbour of bin 0 of the next.
* **Numbering** in the order of each region's smallest cell by ``(recording, frame, bin)``; for reach ``(1, 1)`` that is
  ``scipy.ndimage.label(mask, structure=ones((3, 3)))``.
* **Columns**, one row per region, int32 on the device: ``recording``, ``first_frame``, ``last_frame`` (on the recording's grid,
  inclusive), ``low_bin``, ``high_bin`` (inclusive), ``n_cells``, ``n_frames = last_frame - first_frame + 1``,
  ``n_bins = high_bin - low_bin + 1``.
* **Filters** ``min_cells``, ``min_frames``, ``min_bins`` (>= 1) and ``max_frames`` (``None`` or >= 1): a region that fails one is
  dropped, the kept ones keep their order and are numbered densely; ``n_found`` (a device scalar) counts them before the filter.
* **Derived columns**, float64 by torch on the device, as :mod:`avex_amd.measurements`: ``begin_s = first_frame hop / sr``,
  ``end_s = (last_frame hop + 512) / sr``, ``low_hz = low_bin sr / 512``, ``high_hz = high_bin sr / 512``,
  ``bandwidth_hz = high_hz - low_hz + sr / 512``, ``duration_s = end_s - begin_s``.

A region's row depends on its recording's samples, that recording's ``thr`` row, ``hop``, the band and the reach alone: the same bits on
every run, in any company of recordings and in any order of them, up to the ``recording`` column.  Everything after the compare is
integer arithmetic.  A call reads two integers back, one each: the number of set cells (to size the working memory), then the number of
kept regions (to size the result); everything returned stays on the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi, activity, measurements
from ._capi import check, lib
from ._frames import N_BINS, N_FFT, _number, _tables_on, _to_device, recording_table
from .soundscape import P_FS

__all__ = ["RegionSpec", "Regions", "find_regions", "label_cells", "COLUMNS", "FLOAT_COLUMNS"]

RUN_FRAMES = 64                           # AVEXHIP_REGIONS_RUN_FRAMES
WORDS = 9                                 # AVEXHIP_REGIONS_WORDS
MAX_REACH = (4, 8)                        # AVEXHIP_REGIONS_MAX_RT, AVEXHIP_REGIONS_MAX_RK
COLUMNS = ("recording", "first_frame", "last_frame", "low_bin", "high_bin", "n_cells", "n_frames", "n_bins")
FLOAT_COLUMNS = ("begin_s", "end_s", "low_hz", "high_hz", "bandwidth_hz", "duration_s")
# avexhip_regions_recording and avexhip_regions_rule, field for field
RECORDING_DTYPE = np.dtype([("base", "<i8"), ("n_samples", "<i8"), ("first_frame", "<i8"), ("first_run", "<i4"), ("reserved", "<i4")])
RULE_DTYPE = np.dtype([("rt", "<i4"), ("rk", "<i4"), ("min_cells", "<i4"), ("min_frames", "<i4"), ("min_bins", "<i4"), ("max_frames", "<i4")])


def _count(x: Any, what: str, lo: int, hi: int = (1 << 31) - 1) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{what}={x!r}: an integer in {lo}..{hi} expected")
    return int(x)


def _reach(x: Any) -> Tuple[int, int]:
    try:
        rt, rk = x
    except (TypeError, ValueError) as e:
        raise ValueError(f"reach={x!r}: a (frames, bins) pair expected") from e
    return _count(rt, "reach[0]", 0, MAX_REACH[0]), _count(rk, "reach[1]", 0, MAX_REACH[1])


def _rule(reach: Any, min_cells: Any, min_frames: Any, min_bins: Any, max_frames: Any) -> np.ndarray:
    rule = np.zeros(1, dtype=RULE_DTYPE)
    rule["rt"], rule["rk"] = _reach(reach)
    rule["min_cells"], rule["min_frames"], rule["min_bins"] = _count(min_cells, "min_cells", 1), _count(min_frames, "min_frames", 1), _count(min_bins, "min_bins", 1)
    rule["max_frames"] = -1 if max_frames is None else _count(max_frames, "max_frames", 1)
    return rule


@dataclass(frozen=True)
class RegionSpec:
    """What to look for, checked when made and immutable.

    ``hop``           samples between frames, 32..512
    ``band``          ``None`` (all 257 bins) or one ``(lo_hz, hi_hz)``; checked against the sample rate by :meth:`bins`
    ``snr_db``        how far over the recording's noise spectrum a cell has to stand
    ``min_db``        a lower bound of the threshold in dB re full scale (``None``: none); the whole threshold without a noise spectrum
    ``reach``         ``(frames, bins)`` two set cells may lie apart and still be neighbours, 0..4 and 0..8
    ``min_cells`` ``min_frames`` ``min_bins`` ``max_frames``   the filters (``max_frames=None``: no upper bound)
    """
    hop: int = 128
    band: Optional[Tuple[float, float]] = None
    snr_db: float = 10.0
    min_db: Optional[float] = None
    reach: Tuple[int, int] = (1, 1)
    min_cells: int = 1
    min_frames: int = 1
    min_bins: int = 1
    max_frames: Optional[int] = None

    def __post_init__(self) -> None:
        object.__setattr__(self, "hop", _count(self.hop, "hop", activity.MIN_HOP, N_FFT))
        if self.band is not None:
            object.__setattr__(self, "band", measurements._pair(self.band, "band"))
        object.__setattr__(self, "snr_db", _number(self.snr_db, "snr_db"))
        if self.min_db is not None:
            object.__setattr__(self, "min_db", _number(self.min_db, "min_db"))
        object.__setattr__(self, "reach", _reach(self.reach))
        rule = self.rule                  # the filters' refusals
        object.__setattr__(self, "min_cells", int(rule["min_cells"][0]))
        object.__setattr__(self, "min_frames", int(rule["min_frames"][0]))
        object.__setattr__(self, "min_bins", int(rule["min_bins"][0]))
        if self.max_frames is not None:
            object.__setattr__(self, "max_frames", int(self.max_frames))

    @property
    def rule(self) -> np.ndarray:
        """The one-element ``RULE_DTYPE`` array the device takes."""
        return _rule(self.reach, self.min_cells, self.min_frames, self.min_bins, self.max_frames)

    @property
    def ratio(self) -> np.float32:
        """``float32(10 ** (snr_db / 10))``."""
        with np.errstate(over="ignore"):
            return np.float32(10.0 ** (self.snr_db / 10.0))

    @property
    def floor(self) -> np.float32:
        """``float32(16384 * 10 ** (min_db / 10))``; 0 without ``min_db``."""
        if self.min_db is None:
            return np.float32(0.0)
        with np.errstate(over="ignore"):
            return np.float32(np.float64(P_FS) * np.power(np.float64(10.0), np.float64(self.min_db) / 10.0))

    def bins(self, sr: int) -> Tuple[int, int]:
        """The band as bins ``lo <= k < hi`` at sample rate ``sr``."""
        if self.band is None:
            return 0, N_BINS
        lo, hi = activity.band_bins([self.band], sr)[0]
        return int(lo), int(hi)

    def threshold(self, noise_power: Optional[torch.Tensor], n_rec: int, dev: torch.device) -> torch.Tensor:
        """``thr [n_rec, 257]`` float32 on ``dev`` (see the module docstring)."""
        floor = torch.full((n_rec, N_BINS), float(self.floor), dtype=torch.float32, device=dev)
        if noise_power is None:
            if self.min_db is None:
                raise ValueError("neither noise_power nor spec.min_db: nothing to compare the cells with")
            return floor
        if not isinstance(noise_power, torch.Tensor) or tuple(noise_power.shape) != (n_rec, N_BINS) or not noise_power.is_floating_point():
            raise ValueError(f"noise_power: a float [{n_rec}, {N_BINS}] tensor expected")
        noise = noise_power.to(device=dev, dtype=torch.float32)
        return torch.maximum(noise * torch.full((), float(self.ratio), dtype=torch.float32, device=dev), floor).contiguous()


class Regions(dict):
    """What :func:`find_regions` and :func:`label_cells` return: a dict of device tensors, one row per kept region (:data:`COLUMNS` int32,
    :data:`FLOAT_COLUMNS` float64 -- the latter only where a sample rate is known), with

    ``cells``              ``[total_frames, 9]`` int32, the mask;  ``frame_offsets`` ``[R + 1]`` int64
    ``nonfinite_frames``   ``[R]`` int32 (zeros for :func:`label_cells`)
    ``n_found``            the regions before the filters, an int64 device scalar
    ``sr`` ``hop``         what they were made at (``None`` for :func:`label_cells`)
    """
    cells: torch.Tensor
    frame_offsets: torch.Tensor
    nonfinite_frames: torch.Tensor
    n_found: torch.Tensor
    sr: Optional[int]
    hop: Optional[int]

    def _grid(self) -> Tuple[int, int]:
        if self.sr is None or self.hop is None:
            raise ValueError("these regions come from a bare mask (label_cells): no sample rate and no hop to place them with")
        return int(self.sr), int(self.hop)

    def boxes(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``(recording, start_sample, end_sample, bins [E, 2])`` on the host (this copies, and waits for the stream):
        ``start_sample = first_frame hop``, ``end_sample = last_frame hop + 512``, ``bins = [low_bin, high_bin + 1)`` -- the boxes whose
        frames (:func:`avex_amd.measurements.event_frames`) are exactly ``first_frame .. last_frame``."""
        _, hop = self._grid()
        cols = torch.stack([self[k] for k in ("recording", "first_frame", "last_frame", "low_bin", "high_bin")]).cpu().numpy().astype(np.int64)
        rec, first, last, low, high = cols
        return rec, first * hop, last * hop + N_FFT, np.stack([low, high + 1], axis=1).reshape(-1, 2)

    def measure(self, ws: Any, mspec: Optional[measurements.MeasureSpec] = None, noise_power: Optional[torch.Tensor] = None) -> measurements.Measurements:
        """:func:`avex_amd.measurements.measure_boxes` of the regions' boxes over the windows ``ws`` they were found in (``mspec=None``:
        a ``MeasureSpec`` at the regions' hop): energy, quantile bounds, peaks and SNR of each region."""
        _, hop = self._grid()
        mspec = measurements.MeasureSpec(hop=hop) if mspec is None else mspec
        rec, s0, s1, bins = self.boxes()
        return measurements.measure_boxes(ws, rec, s0, s1, mspec, noise_power=noise_power, bins=bins)

    def as_events(self) -> Dict[str, np.ndarray]:
        """The host dict :func:`avex_amd.measurements.write_raven` reads as events: ``recording``, ``class_id`` (0), ``first``
        (``first_frame``) and ``peak`` (``float(n_cells)``)."""
        rec, first, cells = (self[k].cpu().numpy() for k in ("recording", "first_frame", "n_cells"))
        return {"recording": rec, "class_id": np.zeros(len(rec), dtype=np.int32), "first": first, "peak": cells.astype(np.float64)}

    def as_measurements(self) -> measurements.Measurements:
        """The host dict :func:`avex_amd.measurements.write_raven` reads as measurements: the regions' own bounds."""
        sr, hop = self._grid()
        out = measurements.Measurements({k: self[k].cpu().numpy() for k in ("low_bin", "high_bin", "begin_s", "end_s", "low_hz", "high_hz")})
        out["low_frame"], out["high_frame"] = self["first_frame"].cpu().numpy(), self["last_frame"].cpu().numpy()
        out.sr, out.hop = sr, hop
        return out


def _label(cells: torch.Tensor, offsets: np.ndarray, rule: np.ndarray, sr: Optional[int], hop: Optional[int], nonfinite: torch.Tensor,
           timed: Optional[Any] = None) -> Regions:
    """cells [F, 9] int32 on the device -> Regions.  ``timed(name, launch)``: scripts/regions_bench.py's hook around each entry point."""
    dev = cells.device
    F, R = int(offsets[-1]), len(offsets) - 1
    L = lib()
    run = (lambda name, launch: launch()) if timed is None else timed
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        pinned, offsets_dev = _to_device(np.ascontiguousarray(offsets, dtype=np.int64), dev)
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
        ptr = lambda t: t.data_ptr() if t.numel() else None
        fbytes = int(L.avexhip_regions_workspace_bytes(F, 0))
        frame_ws = torch.empty(fbytes // 8 + 1, dtype=torch.int64, device=dev)
        run("count", lambda: check(L.avexhip_regions_count(ptr(cells), F, frame_ws.data_ptr(), fbytes, counts.data_ptr(), stream), "regions_count"))
        n_cells = int(counts[0].item())                           # the first of the two host reads
        cbytes = int(L.avexhip_regions_workspace_bytes(0, n_cells)) if n_cells < 1 << 31 else 0
        cell_ws = torch.empty(cbytes // 8 + 1, dtype=torch.int64, device=dev)
        run("label", lambda: check(L.avexhip_regions_label(ptr(cells), offsets.ctypes.data, offsets_dev.view(torch.int64).data_ptr(), R, F, n_cells,
                                                           rule.ctypes.data, frame_ws.data_ptr(), fbytes, cell_ws.data_ptr(), cbytes, counts.data_ptr(), stream),
                                   "regions_label"))
        n_kept = int(counts[2].item())                            # the second
        rows = torch.empty((len(COLUMNS), n_kept), dtype=torch.int32, device=dev)
        run("rows", lambda: check(L.avexhip_regions_rows(n_cells, n_kept, rule.ctypes.data, cell_ws.data_ptr(), cbytes, counts.data_ptr(), ptr(rows), stream),
                                  "regions_rows"))
        out = Regions({name: rows[c] for c, name in enumerate(COLUMNS)})
        if sr is not None and hop is not None:
            first, last = out["first_frame"].to(torch.int64), out["last_frame"].to(torch.int64)
            rate = torch.full((), float(sr), dtype=torch.float64, device=dev)      # a tensor: a true division (by a Python number torch multiplies by 1 / sr)
            out["begin_s"] = (first * hop).to(torch.float64) / rate
            out["end_s"] = (last * hop + N_FFT).to(torch.float64) / rate
            out["low_hz"] = out["low_bin"].to(torch.float64) * sr / N_FFT
            out["high_hz"] = out["high_bin"].to(torch.float64) * sr / N_FFT
            out["bandwidth_hz"] = out["high_hz"] - out["low_hz"] + sr / N_FFT
            out["duration_s"] = out["end_s"] - out["begin_s"]
        out.cells, out.frame_offsets, out.nonfinite_frames, out.n_found = cells, offsets_dev.view(torch.int64), nonfinite, counts[1]
        out.n_cells = n_cells
        out.sr, out.hop, out._keep = sr, hop, [pinned, frame_ws, cell_ws, counts]
    return out


def find_regions(ws: Any, spec: Optional[RegionSpec] = None, *, noise_power: Optional[torch.Tensor] = None, _timed: Optional[Any] = None) -> Regions:
    """The regions of the recordings behind the windows ``ws`` (a :class:`~avex_amd.recordings.RecordingWindows`; its window plan plays
    no part) under ``spec``.  ``noise_power [R, 257]``: a device tensor, e.g.
    ``measurements.noise_spectrum(soundscape.spectral_stats(ws, ...))``; without it ``spec.min_db`` is the threshold.  See the module
    docstring for what comes back."""
    spec = RegionSpec() if spec is None else spec
    if not isinstance(spec, RegionSpec):
        raise TypeError(f"a RegionSpec expected, not {type(spec).__name__}")
    sr, hop = int(ws.sr), spec.hop
    lo, hi = spec.bins(sr)                # a band the sample rate cannot hold raises here, before anything is launched
    rec, frames = recording_table(ws, RECORDING_DTYPE, hop)
    runs = (frames + RUN_FRAMES - 1) // RUN_FRAMES
    rec["first_run"] = np.cumsum(runs) - runs
    F, R = int(frames.sum()), len(rec)
    if max(F, int(runs.sum())) >= 1 << 31:
        raise ValueError(f"{F} frames: more than 2^31 - 1 (a longer hop, or fewer recordings per call)")
    offsets = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(frames, out=offsets[1:])
    _capi.require_gpu()
    dev = ws.wav.device
    thr = spec.threshold(noise_power, R, dev)
    run = (lambda name, launch: launch()) if _timed is None else _timed
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        pinned, rec_dev = _to_device(rec, dev)
        cells = torch.empty((F, WORDS), dtype=torch.int32, device=dev)
        nonfinite = torch.empty(R, dtype=torch.int32, device=dev)
        tab = _tables_on(dev)
        run("cells", lambda: check(lib().avexhip_regions_cells(ws.wav.data_ptr(), ws.wav.numel(), rec.ctypes.data, rec_dev.data_ptr(), R, hop, lo, hi, thr.data_ptr(),
                                                               tab.data_ptr(), F, cells.data_ptr() if F else None, nonfinite.data_ptr(), stream), "regions_cells"))
    out = _label(cells, offsets, spec.rule, sr, hop, nonfinite, _timed)
    out._keep += [pinned, rec_dev, thr]
    return out


def label_cells(mask: torch.Tensor, frames_per_recording: Sequence[int], reach: Tuple[int, int] = (1, 1), *, min_cells: int = 1, min_frames: int = 1,
                min_bins: int = 1, max_frames: Optional[int] = None) -> Regions:
    """The regions of a ``[total_frames, 257]`` bool device tensor from anywhere -- the labelling kernels of :func:`find_regions`
    without its cells kernel.  ``frames_per_recording``: how many of the mask's rows each recording holds, in order (a region never
    crosses from one into the next).  No sample rate and no hop: the float columns and :meth:`Regions.boxes` are not available."""
    rule = _rule(reach, min_cells, min_frames, min_bins, max_frames)
    frames = np.asarray(list(frames_per_recording))
    if frames.ndim != 1 or len(frames) < 1 or frames.dtype.kind not in "iu" or (frames < 0).any():
        raise ValueError("frames_per_recording: at least one integer >= 0 expected")
    offsets = np.zeros(len(frames) + 1, dtype=np.int64)
    np.cumsum(frames.astype(np.int64), out=offsets[1:])
    F = int(offsets[-1])
    if F >= 1 << 31:
        raise ValueError(f"{F} frames: more than 2^31 - 1")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (F, N_BINS):
        raise ValueError(f"mask: a bool [{F}, {N_BINS}] tensor expected ({F} = the sum of frames_per_recording)")
    _capi.require_gpu()
    if not mask.is_cuda:
        raise ValueError("mask: a device tensor expected")
    dev = mask.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        bytes_ = mask.contiguous().view(torch.uint8)
        cells = torch.empty((F, WORDS), dtype=torch.int32, device=dev)
        check(lib().avexhip_regions_pack(bytes_.data_ptr() if F else None, F, cells.data_ptr() if F else None, stream), "regions_pack")
        nonfinite = torch.zeros(len(frames), dtype=torch.int32, device=dev)
    out = _label(cells, offsets, rule, None, None, nonfinite)
    out._keep.append(bytes_)
    return out
