"""Whole-recording embedding: every sliding window of a long recording, an energy gate, one embedding per kept window.

The rest of the package inherits the reference's evaluation view of audio -- one clip, one window: ``pad_or_window`` crops a long clip to a
single ``start`` / ``center`` / ``random`` window (avex/data/audio_utils.py:16-73) and drops the rest, and the step that would say which
windows are worth embedding is a name without a body (avex/preprocessing/activity_detector.py is empty; its long-audio wrappers chunk by
hand; :mod:`avex_amd.activity` is that step here, the ``activity=`` gate of the functions below).  Here a recording is decoded, averaged
to mono and resampled ONCE (:func:`avex_amd.ingest.load_audio`'s pieces) and stays on the device; three kernels of ``csrc/windows.hip``
read that resident waveform through a table of ``(recording, start, valid)``:

* ``avexhip_window_stats``   per window the peak ``max |x|`` and the energy ``sum x^2`` (fp64), in an order that depends on the window alone;
* ``avexhip_window_select``  windows over two thresholds -> their numbers in increasing order and the count (prefix sum, no atomics);
* ``avexhip_window_gather``  the padded rows and padding masks of a list, or a range, of windows in one launch.

A window row is what the reference's ``pad_or_window(wav[start:], window_len, "start")`` returns: the samples, then zeros, mask ``True`` on
the padding -- bit for bit the row :func:`avex_amd.ingest.load_batch` gives for the same file and start.  Unlike ``load_batch``, a NaN or
Inf sample is not zeroed: it stays in its windows, whose energy is NaN and which no gate keeps.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi, _frames, ingest
from ._capi import check, lib

__all__ = ["plan_recording_windows", "RecordingWindows", "windows", "embed_recording", "embed_recordings"]

TAILS = ("pad", "drop")
MAX_RESIDENT_SAMPLES = 1 << 28            # 1 GiB of fp32: 4.6 hours at 16 kHz
# avexhip_window, field for field
WINDOW_DTYPE = np.dtype([("base", "<i8"), ("n_samples", "<i8"), ("start", "<i8"), ("valid", "<i4"), ("reserved", "<i4")])
_MAX_ROWS = 65535                         # rows of one avexhip_window_gather launch


def plan_recording_windows(n_samples: int, window_len: int, hop_len: int, tail: str = "pad") -> Tuple[np.ndarray, np.ndarray]:
    """``(starts, valids)`` (int64) of the sliding windows over ``n_samples`` samples: windows start at ``0, hop, 2 hop, ...`` while
    ``start < n_samples``.  ``tail="pad"`` keeps the last, short windows (``valid < window_len``); ``tail="drop"`` keeps full windows only,
    except that a recording shorter than one window still gives exactly one padded window, so a short file embeds."""
    n, w, h = int(n_samples), int(window_len), int(hop_len)
    if n <= 0 or w <= 0 or h <= 0:
        raise ValueError(f"n_samples={n_samples}, window_len={window_len}, hop_len={hop_len}: positive lengths expected")
    if tail not in TAILS:
        raise ValueError(f"Unknown tail: {tail!r} (one of {TAILS})")
    count = (n - 1) // h + 1 if tail == "pad" else max((n - w) // h + 1, 1)
    starts = np.arange(count, dtype=np.int64) * h
    return starts, np.minimum(w, n - starts)


def _to_len(seconds: float, sr: int, what: str) -> int:
    n = int(round(float(seconds) * sr))
    if n <= 0:
        raise ValueError(f"{what}={seconds} s is no sample at {sr} Hz")
    return n


def _resident(source: Any, sr: int, res_type: Optional[str], dev: torch.device, max_resident_samples: int) -> torch.Tensor:
    """One source -> its mono float32 waveform at ``sr`` on the device: ``load_audio``'s pieces, with ``res_type`` and array sources."""
    e = ingest._open_source(source, sr)
    rs, n = None, e.frames
    if e.sr != sr:
        key = (e.sr, sr, res_type)
        if key not in ingest._BATCH_RESAMPLERS:
            ingest._BATCH_RESAMPLERS[key] = ingest.Resampler(e.sr, sr, res_type=res_type)
        rs = ingest._BATCH_RESAMPLERS[key]
        n = rs.out_length(e.frames)
    if n > max_resident_samples:
        raise ValueError(f"the recording holds {n} samples at {sr} Hz, more than max_resident_samples={max_resident_samples}: "
                         "split the file (a recording is embedded from one waveform resident on the device)")
    if e.flac is not None:
        pcm = e.flac.decode(dev, left_justify=True)
        x = ingest.to_device_mono(pcm, e.channels, 32, dev)
        e.flac.close()
    else:
        x = ingest.to_device_mono(e.payload[:e.nbytes], e.channels, e.fmt, dev)
    return x if rs is None else rs(x)


class RecordingWindows:
    """The sliding windows of one or more recordings over their resident waveforms.

    ``wav``                    the waveforms, back to back (each at a 16-byte aligned offset), float32 on the device
    ``starts`` ``valids``      the host plan (int64); ``start_s`` / ``end_s`` the span of each window's samples in seconds (float64)
    ``recording``              which source a window belongs to; ``ranges[r]`` = the windows ``[w0, w1)`` of source ``r``
    ``energy`` ``peak``        ``sum x^2`` over the valid samples (float64) and ``max |x|`` (float32) per window, on the device
    ``rms_db`` ``peak_db``     ``10 log10(energy / valid)`` and ``20 log10(peak)`` on the host in float64 (``-inf`` for silence, NaN for
                               a window that holds a NaN or an Inf); the first access copies the statistics from the device
    ``batch(lo, hi)`` / ``batch(index)``   ``(wav [B, window_len] float32, padding_mask [B, window_len] bool)`` on the device
    """

    def __init__(self, waves: Sequence[torch.Tensor], sr: int, window_len: int, hop_len: int, tail: str = "pad") -> None:
        if len(waves) == 0:
            raise ValueError("no recordings")
        _capi.require_gpu()
        self.sr, self.window_len, self.hop_len, self.tail = int(sr), int(window_len), int(hop_len), tail
        dev = waves[0].device
        plans = [plan_recording_windows(int(x.numel()), window_len, hop_len, tail) for x in waves]
        bases, pos = [], 0
        for x in waves:
            bases.append(pos)
            pos = (pos + int(x.numel()) + 3) & ~3
        if len(waves) == 1:
            self.wav = waves[0].contiguous()
        else:
            self.wav = torch.empty(pos, dtype=torch.float32, device=dev)          # the gaps are never read
            for b, x in zip(bases, waves):
                self.wav[b:b + x.numel()].copy_(x)
        self.ranges: List[Tuple[int, int]] = []
        n = 0
        for s, _ in plans:
            self.ranges.append((n, n + len(s)))
            n += len(s)
        if n >= 1 << 31:
            raise ValueError(f"{n} windows: more than 2^31 - 1 (a longer hop, or fewer recordings per call)")
        self.n_windows = n
        self.starts = np.concatenate([s for s, _ in plans])
        self.valids = np.concatenate([v for _, v in plans])
        self.recording = np.concatenate([np.full(len(s), r, dtype=np.int32) for r, (s, _) in enumerate(plans)])
        self.start_s = self.starts.astype(np.float64) / self.sr
        self.end_s = (self.starts + self.valids).astype(np.float64) / self.sr
        self._table = np.zeros(n, dtype=WINDOW_DTYPE)
        self._table["base"] = np.asarray(bases, dtype=np.int64)[self.recording]
        self._table["n_samples"] = np.asarray([x.numel() for x in waves], dtype=np.int64)[self.recording]
        self._table["start"], self._table["valid"] = self.starts, self.valids
        with torch.cuda.device(dev):
            self._table_pinned, self._table_dev = _frames._to_device(self._table, dev)      # the pinned copy is kept: the device copy is asynchronous
            self.energy = torch.empty(n, dtype=torch.float64, device=dev)
            self.peak = torch.empty(n, dtype=torch.float32, device=dev)
            check(lib().avexhip_window_stats(self.wav.data_ptr(), self.wav.numel(), self._table.ctypes.data, self._table_dev.data_ptr(), n, self.window_len,
                                             self.energy.data_ptr(), self.peak.data_ptr(), torch.cuda.current_stream().cuda_stream), "window_stats")
        self._db: Optional[Tuple[np.ndarray, np.ndarray]] = None

    def __len__(self) -> int:
        return self.n_windows

    def _host_db(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._db is None:
            e, p = self.energy.cpu().numpy(), self.peak.cpu().numpy().astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                self._db = (10.0 * np.log10(e / self.valids), 20.0 * np.log10(p))
        return self._db

    @property
    def rms_db(self) -> np.ndarray:
        return self._host_db()[0]

    @property
    def peak_db(self) -> np.ndarray:
        return self._host_db()[1]

    def _device_db(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``rms_db`` / ``peak_db`` as float64 device tensors, without a copy to the host (the ``valid`` column of the resident table)."""
        valid = self._table_dev.view(torch.int32).view(-1, WINDOW_DTYPE.itemsize // 4)[:, 6].to(torch.float64)
        return 10.0 * torch.log10(self.energy / valid), 20.0 * torch.log10(self.peak.to(torch.float64))

    def select(self, min_rms_db: Optional[float] = None, min_peak_db: Optional[float] = None) -> torch.Tensor:
        """int32 ``[n_windows + 1]`` on the device, no copy to the host: ``[n_windows]`` holds the count ``k`` of windows with
        ``rms_db >= min_rms_db`` and ``peak_db >= min_peak_db`` (``None``: that threshold is off), ``[:k]`` their numbers in increasing
        order.  The thresholds reach the device as mean-square and amplitude numbers computed here."""
        thr_e = -math.inf if min_rms_db is None else 10.0 ** (float(min_rms_db) / 10.0)
        thr_p = -math.inf if min_peak_db is None else 10.0 ** (float(min_peak_db) / 20.0)
        n = self.n_windows
        with torch.cuda.device(self.wav.device):
            out = torch.empty(n + 1, dtype=torch.int32, device=self.wav.device)
            check(lib().avexhip_window_select(self._table_dev.data_ptr(), self.energy.data_ptr(), self.peak.data_ptr(), n, thr_e, thr_p, out.data_ptr(),
                                              out.data_ptr() + 4 * n, torch.cuda.current_stream().cuda_stream), "window_select")
        return out

    def _gather(self, index: Optional[torch.Tensor], first: int, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.wav.device
        with torch.cuda.device(dev):
            wav = torch.empty((rows, self.window_len), dtype=torch.float32, device=dev)
            mask = torch.empty((rows, self.window_len), dtype=torch.bool, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            for r0 in range(0, rows, _MAX_ROWS):
                nb = min(_MAX_ROWS, rows - r0)
                check(lib().avexhip_window_gather(self.wav.data_ptr(), self.wav.numel(), self._table.ctypes.data, self._table_dev.data_ptr(), self.n_windows,
                                                  index.data_ptr() + 4 * r0 if index is not None else None, first + r0, nb, self.window_len,
                                                  wav[r0:].data_ptr(), self.window_len, mask[r0:].data_ptr(), stream), "window_gather")
        return wav, mask

    def batch(self, lo: Union[int, torch.Tensor, np.ndarray, Sequence[int]], hi: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Rows and padding masks of the windows ``lo .. hi - 1``, or of the window numbers in an index tensor (any order, repeats
        allowed).  A host index is checked here; in a device index, which is not copied back, a number outside the table gives a zero
        row that is all padding."""
        dev = self.wav.device
        if isinstance(lo, (int, np.integer)):
            lo, hi = int(lo), self.n_windows if hi is None else int(hi)
            if not 0 <= lo <= hi <= self.n_windows:
                raise IndexError(f"windows {lo}..{hi} outside 0..{self.n_windows}")
            if lo == hi:
                return torch.empty((0, self.window_len), dtype=torch.float32, device=dev), torch.empty((0, self.window_len), dtype=torch.bool, device=dev)
            return self._gather(None, lo, hi - lo)
        if hi is not None:
            raise TypeError("batch(index) takes no second argument")
        idx = lo if isinstance(lo, torch.Tensor) else torch.as_tensor(np.asarray(lo))
        if idx.dim() != 1 or idx.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise TypeError("a 1-d integer index is expected")
        if idx.numel() == 0:
            return torch.empty((0, self.window_len), dtype=torch.float32, device=dev), torch.empty((0, self.window_len), dtype=torch.bool, device=dev)
        if not idx.is_cuda and (int(idx.min()) < 0 or int(idx.max()) >= self.n_windows):
            raise IndexError(f"window index outside 0..{self.n_windows - 1}")
        idx = idx.to(device=dev, dtype=torch.int32).contiguous()
        return self._gather(idx, 0, int(idx.numel()))


def _device_of(device: Any) -> torch.device:
    _capi.require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _capi.AvexHipError(f"recordings live on a GPU, not on {dev} (there is no CPU fallback)")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _windows_of(sources: Sequence[Any], window_s: float, hop_s: Optional[float], sr: int, tail: str, res_type: Optional[str], device: Any,
                max_resident_samples: int) -> RecordingWindows:
    if tail not in TAILS:
        raise ValueError(f"Unknown tail: {tail!r} (one of {TAILS})")
    sr = int(sr)
    window_len = _to_len(window_s, sr, "window_s")
    hop_len = window_len if hop_s is None else _to_len(hop_s, sr, "hop_s")
    dev = _device_of(device)
    with torch.cuda.device(dev):
        waves = [_resident(s, sr, res_type, dev, int(max_resident_samples)) for s in sources]
    return RecordingWindows(waves, sr, window_len, hop_len, tail)


def windows(source: Any, window_s: float, hop_s: Optional[float] = None, *, sr: int = 16000, tail: str = "pad", res_type: Optional[str] = None,
            device: Any = None, max_resident_samples: int = MAX_RESIDENT_SAMPLES) -> RecordingWindows:
    """The sliding windows of one recording: ``source`` is a path or bytes (WAV / FLAC, resampled to ``sr``; ``res_type`` as
    :class:`avex_amd.ingest.Resampler` takes it) or a ``(T,)`` / ``(C, T)`` array at ``sr``; windows of ``window_s`` seconds every ``hop_s``
    (``None``: no overlap); ``tail`` as :func:`plan_recording_windows`.  The waveform stays on the device, so a recording of more than
    ``max_resident_samples`` samples raises ``ValueError``: split the file."""
    return _windows_of([source], window_s, hop_s, sr, tail, res_type, device, max_resident_samples)


def _embed(model: Any, ws: RecordingWindows, layers: Optional[Sequence[Any]], aggregation: str, batch_size: int, min_rms_db: Optional[float],
           min_peak_db: Optional[float], batch_invariant: Optional[bool], activity: Optional[Any] = None) -> List[Dict[str, Any]]:
    if int(batch_size) <= 0:
        raise ValueError(f"batch_size={batch_size}: a positive number of windows expected")
    batch_size = min(int(batch_size), _MAX_ROWS)
    if batch_invariant is not None and hasattr(model, "batch_invariant") and bool(model.batch_invariant) != bool(batch_invariant):
        model.batch_invariant = bool(batch_invariant)
        model._weights_dirty = True      # the next forward builds its handle again, with the other policy (as extract_embeddings_in_memory)
    if layers is not None:
        model.register_hooks_for_layers(list(layers))
    elif not model._hook_layers:
        model.register_hooks_for_layers(["last_layer"])
    else:
        model.ensure_hooks_registered()
    n = ws.n_windows
    gated = min_rms_db is not None or min_peak_db is not None or activity is not None
    kept_dev, kept, act = None, np.arange(n, dtype=np.int64), None
    if activity is not None:
        from .activity import band_activity
        act = band_activity(ws, activity)
    if gated:
        kept_dev = ws.select(min_rms_db, min_peak_db) if act is None else act.select(min_rms_db, min_peak_db)
        host = kept_dev.cpu().numpy()                             # the call's one host synchronisation: the count, and the list with it
        kept = host[:int(host[n])].astype(np.int64)
    chunks: List[Any] = []
    with torch.no_grad():
        for lo in range(0, len(kept), batch_size):
            hi = min(lo + batch_size, len(kept))
            wav, mask = ws._gather(kept_dev[lo:hi], 0, hi - lo) if gated else ws._gather(None, lo, hi - lo)
            chunks.append(model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation=aggregation))
    if not chunks:
        emb: Any = torch.empty((0,), dtype=torch.float32, device=ws.wav.device)      # nothing ran, so the embedding shape is unknown
    elif isinstance(chunks[0], (list, tuple)):                    # aggregation="none" with several layers: one tensor per layer
        emb = [torch.cat([c[i] for c in chunks]) for i in range(len(chunks[0]))]
    else:
        emb = torch.cat(chunks)
    rms_db, peak_db = ws._device_db()
    out = []
    for r, (w0, w1) in enumerate(ws.ranges):
        a, b = (int(v) for v in np.searchsorted(kept, [w0, w1]))
        idx = kept[a:b]
        flags = np.zeros(w1 - w0, dtype=bool)
        flags[idx - w0] = True
        out.append({"embeddings": [e[a:b] for e in emb] if isinstance(emb, list) else emb[a:b],
                    "window_index": torch.from_numpy(idx - w0), "start_s": ws.start_s[idx], "end_s": ws.end_s[idx],
                    "kept": torch.from_numpy(flags), "rms_db": rms_db[w0:w1], "peak_db": peak_db[w0:w1]})
        if act is not None:
            out[-1].update(active_frames=act.active_frames[w0:w1], floor=act.floor[r])
    return out


def embed_recordings(model: Any, sources: Sequence[Any], window_s: float, hop_s: Optional[float] = None, *, layers: Optional[Sequence[Any]] = None,
                     aggregation: str = "mean", batch_size: int = 256, min_rms_db: Optional[float] = None, min_peak_db: Optional[float] = None,
                     tail: str = "pad", batch_invariant: Optional[bool] = None, sr: int = 16000, res_type: Optional[str] = None, device: Any = None,
                     max_resident_samples: int = MAX_RESIDENT_SAMPLES, activity: Optional[Any] = None) -> List[Dict[str, Any]]:
    """:func:`embed_recording` over several recordings whose windows share the batches, so short files still fill them; one dict per
    source, in order, each with the bits the single-source call gives when the model is batch invariant."""
    if len(sources) == 0:
        raise ValueError("no recordings")
    if device is None and isinstance(model, torch.nn.Module):
        p = next(model.parameters(), None)
        device = p.device if p is not None and p.is_cuda else None
    ws = _windows_of(list(sources), window_s, hop_s, sr, tail, res_type, device, max_resident_samples)
    return _embed(model, ws, layers, aggregation, batch_size, min_rms_db, min_peak_db, batch_invariant, activity)


def embed_recording(model: Any, source: Any, window_s: float, hop_s: Optional[float] = None, *, layers: Optional[Sequence[Any]] = None,
                    aggregation: str = "mean", batch_size: int = 256, min_rms_db: Optional[float] = None, min_peak_db: Optional[float] = None,
                    tail: str = "pad", batch_invariant: Optional[bool] = None, sr: int = 16000, res_type: Optional[str] = None, device: Any = None,
                    max_resident_samples: int = MAX_RESIDENT_SAMPLES, activity: Optional[Any] = None) -> Dict[str, Any]:
    """One embedding per window of a recording, for any ``ModelBase`` of the package (only ``register_hooks_for_layers`` and
    ``extract_embeddings({"raw_wav", "padding_mask"}, aggregation=...)`` are used).

    ``layers``: registered when given; ``None`` keeps what is registered, or takes the model's last layer.  ``min_rms_db`` /
    ``min_peak_db`` (dB re full scale; ``None``: off) gate the windows by their statistics before any of them reaches the model;
    ``activity`` (an :class:`avex_amd.activity.ActivityGate`; ``None``: off) adds its band condition to that gate and the keys
    ``active_frames`` (``[n_windows, n_bands]`` int32) and ``floor`` (``[n_bands]`` float32), on the device.
    ``batch_invariant`` as :func:`avex_amd.extraction.extract_embeddings_in_memory` takes it: with ``True`` a window's embedding does not
    depend on ``batch_size`` or on the windows beside it.  Returns

    ``embeddings``     ``[n_kept, ...]`` on the device (a list of such tensors for ``aggregation="none"`` with several layers; an empty
                       ``[0]`` tensor when the gate keeps nothing)
    ``window_index``   ``[n_kept]`` int64, the kept windows' numbers;  ``start_s`` / ``end_s``: their spans in seconds (float64)
    ``kept``           ``[n_windows]`` bool;  ``rms_db`` / ``peak_db``: ``[n_windows]`` float64 on the device, for ALL windows

    With a gate the only host synchronisation is the copy of the kept list, once per call; without one there is none."""
    return embed_recordings(model, [source], window_s, hop_s, layers=layers, aggregation=aggregation, batch_size=batch_size, min_rms_db=min_rms_db,
                            min_peak_db=min_peak_db, tail=tail, batch_invariant=batch_invariant, sr=sr, res_type=res_type, device=device,
                            max_resident_samples=max_resident_samples, activity=activity)[0]
