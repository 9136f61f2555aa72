"""Event detection over recordings: one score per (window, class) -> "class c is present from 12.5 s to 17.0 s of recording r, peak 0.93".

:func:`avex_amd.recordings.embed_recordings` leaves one embedding per sliding window on the device and a probe turns them into an
``[N, C]`` score matrix; the step after that -- the one the reference names and leaves empty (avex/preprocessing/activity_detector.py has no
body) -- is here.  :func:`decode_events` takes the scores where they are and returns the events as device tensors; :func:`detect_events`
runs the whole chain from files.  The arithmetic is in ``libavexhip.so`` (``csrc/events.hip``); there is no CPU fallback.

Semantics (the tests hold them; ``tests/_detection_ref.py`` restates them in NumPy).  Per sequence (one recording's windows in time order)
and class, on fp32 scores, a window without a score being NaN:

1. **Smoothing** (``smooth`` odd, 1..31): over the positions ``i - h .. i + h`` inside the sequence that hold a number; ``"median"`` is the
   lower median (element ``(n - 1) // 2`` of the sorted numbers), ``"mean"`` the fp32 sum in position order over ``float(n)``; none: NaN.
2. **Hysteresis** from inactive: ``s >= on[c]`` sets, ``not (s >= off[c])`` clears (so NaN clears), anything else holds.
3. **Merge** (``merge_gap`` 0..64): an inactive run of at most ``merge_gap`` windows strictly between two active runs becomes active.
4. **Minimum length** (``min_windows`` 1..64): active runs shorter than that are dropped.

An event is a remaining maximal run: ``sequence``, ``class_id``, ``first`` / ``last`` (global window numbers), ``peak`` (the largest
smoothed score), ``peak_window`` (the lowest window attaining it), ``mean`` (float64, over the smoothed scores that are numbers).  Events
come sorted by ``(sequence, class_id, first)``; every column but ``mean`` is known bit for bit, and ``mean`` has the same bits on every
run and for every ``max_events``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Any, Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._metric_inputs import _as_tensor, _stream

MAX_SMOOTH = 31                 # avexhip_events_max_smooth()
MAX_SPAN = 64                   # avexhip_events_max_span(): the largest merge_gap and min_windows
MAX_WINDOWS = (1 << 31) - 1
SMOOTH_MODES = ("median", "mean")
ACTIVATIONS = (None, "sigmoid")
COLUMNS = (("sequence", torch.int32), ("class_id", torch.int32), ("first", torch.int32), ("last", torch.int32), ("peak", torch.float32),
           ("peak_window", torch.int32), ("mean", torch.float64))

__all__ = ["decode_events", "detect_events", "MAX_SMOOTH", "MAX_SPAN"]


def _int_in(x, lo: int, hi: int, what: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{what}={x!r}: an integer in {lo}..{hi} expected")
    return int(x)


def _check_rules(smooth, smooth_mode, merge_gap, min_windows, max_events, activation) -> None:
    if _int_in(smooth, 1, MAX_SMOOTH, "smooth") % 2 == 0:
        raise ValueError(f"smooth={smooth!r}: an odd number of windows expected")
    if smooth_mode not in SMOOTH_MODES:
        raise ValueError(f"smooth_mode={smooth_mode!r}: one of {SMOOTH_MODES} expected")
    _int_in(merge_gap, 0, MAX_SPAN, "merge_gap")
    _int_in(min_windows, 1, MAX_SPAN, "min_windows")
    if max_events is not None:
        _int_in(max_events, 0, 1 << 40, "max_events")
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation={activation!r}: one of {ACTIVATIONS} expected")


def _thresholds(on, off, n_classes: Optional[int], activation) -> tuple:
    """``on`` / ``off`` (scalars or [C] arrays; ``off=None``: ``on``) -> two fp32 arrays, checked; ``n_classes=None``: as many as given."""
    if on is None:
        raise ValueError("on: a threshold, or one per class, expected")
    cols = []
    for name, x in (("on", on), ("off", on if off is None else off)):
        a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
        if a.dtype.kind not in "iuf" or a.ndim > 1:
            raise ValueError(f"{name}: a number or a 1-d array of numbers expected")
        a = a.astype(np.float64)
        if n_classes is not None:
            if a.ndim == 1 and a.shape[0] != n_classes:
                raise ValueError(f"{name} holds {a.shape[0]} thresholds for {n_classes} classes")
            a = np.broadcast_to(a, (n_classes,))
        a = np.atleast_1d(a)
        if np.isnan(a).any():
            raise ValueError(f"{name} holds a NaN")
        if activation == "sigmoid":
            if not ((a > 0.0) & (a < 1.0)).all():
                raise ValueError(f"{name}: probabilities in (0, 1) expected with activation='sigmoid'")
            a = np.log(a / (1.0 - a))                 # the kernels stay in score space: thresholds become logits, in fp64
        cols.append(np.ascontiguousarray(a.astype(np.float32)))
    t_on, t_off = np.broadcast_arrays(*cols)
    if (t_off > t_on).any():
        c = int(np.argmax(t_off > t_on))
        raise ValueError(f"off > on for class {c} ({t_off[c]} > {t_on[c]}): hysteresis needs off <= on")
    return np.ascontiguousarray(t_on), np.ascontiguousarray(t_off)


def _offsets(seq_offsets, windows, n: Optional[int]) -> np.ndarray:
    if seq_offsets is not None and windows is not None:
        raise ValueError("seq_offsets and windows: one of the two, not both")
    if windows is not None:
        off = np.asarray([w0 for w0, _ in windows.ranges] + [windows.ranges[-1][1]], dtype=np.int64)
    elif seq_offsets is None:
        off = np.asarray([0, 0 if n is None else n], dtype=np.int64)                                # one sequence
    else:
        a = np.asarray(seq_offsets.detach().cpu() if isinstance(seq_offsets, torch.Tensor) else seq_offsets)
        if a.ndim != 1 or a.shape[0] < 2 or a.dtype.kind not in "iu":
            raise ValueError("seq_offsets: a 1-d integer array of R + 1 >= 2 entries expected")
        off = a.astype(np.int64)
    if off[0] != 0:
        raise ValueError(f"seq_offsets[0] = {int(off[0])}, not 0")
    if (np.diff(off) < 0).any():
        r = int(np.argmax(np.diff(off) < 0))
        raise ValueError(f"seq_offsets[{r + 1}] = {int(off[r + 1])} < seq_offsets[{r}] = {int(off[r])}")
    if n is not None and off[-1] != n:
        raise ValueError(f"seq_offsets ends at {int(off[-1])}, not at the {n} windows")
    return np.ascontiguousarray(off)


def _to_device(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    """A small host array -> the device through pinned memory, without waiting for it."""
    return torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)


def _empty(dev, cap: int, activation, windows) -> Dict[str, torch.Tensor]:
    fill = {torch.int32: -1, torch.float32: -math.inf, torch.float64: math.nan}
    out = {name: torch.full((cap,), fill[dt], dtype=dt, device=dev) for name, dt in COLUMNS}
    out["count"] = torch.zeros((), dtype=torch.int64, device=dev)
    return _derived(out, activation, windows)


def _derived(out: Dict[str, torch.Tensor], activation, windows) -> Dict[str, torch.Tensor]:
    """The columns torch makes of the seven: n_windows, peak_prob, and with ``windows`` the recording and the times."""
    valid = out["first"] >= 0
    out["n_windows"] = torch.where(valid, out["last"] - out["first"] + 1, torch.full_like(out["first"], -1))
    if activation == "sigmoid":
        out["peak_prob"] = torch.sigmoid(out["peak"])
    if windows is not None:
        dev = out["first"].device
        nan = torch.full((), math.nan, dtype=torch.float64, device=dev)
        start, end = _to_device(np.ascontiguousarray(windows.start_s), dev), _to_device(np.ascontiguousarray(windows.end_s), dev)
        top = max(windows.n_windows - 1, 0)
        out["recording"] = out["sequence"].clone()
        out["start_s"] = torch.where(valid, start[out["first"].clamp(0, top).long()], nan)
        out["end_s"] = torch.where(valid, end[out["last"].clamp(0, top).long()], nan)
        out["peak_s"] = torch.where(valid, start[out["peak_window"].clamp(0, top).long()], nan)
    return out


def decode_events(scores, *, seq_offsets=None, windows=None, on=None, off=None, activation: Optional[str] = None, smooth: int = 1,
                  smooth_mode: str = "median", merge_gap: int = 0, min_windows: int = 1, row_of_window=None,
                  max_events: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Scores ``[M, C]`` (NumPy or torch, any float dtype, host or device; a device tensor is never copied to the host) -> events.

    ``seq_offsets [R + 1]``: the windows of sequence ``r`` are ``[off[r], off[r + 1])`` (``None``: one sequence), or ``windows``: a
    :class:`avex_amd.recordings.RecordingWindows`, which supplies the offsets and adds ``recording``, ``start_s`` (the start of ``first``),
    ``end_s`` (the end of ``last``) and ``peak_s`` (the start of the peak window), float64, gathered on the device.  ``row_of_window [N]``
    (int): the score row of each window, ``-1`` for a window without a score (an energy gate dropped it); without it ``M == N``.
    ``on`` / ``off``: a threshold or one per class (``off=None``: ``on``); with ``activation="sigmoid"`` they are probabilities in (0, 1),
    turned into logits here, and a ``peak_prob = sigmoid(peak)`` column is added -- the kernels stay in score space.

    Returns device tensors ``sequence``, ``class_id``, ``first``, ``last``, ``peak_window``, ``n_windows`` (int32), ``peak`` (float32),
    ``mean`` (float64) and ``count`` (int64 scalar, the true number of events).  ``max_events=None`` reads ``count`` once (the call's one
    host synchronisation) and allocates exactly; an integer gives buffers of that many rows and no synchronisation, the first
    ``max_events`` events, and past ``min(count, max_events)`` ``-1`` / ``-inf`` / NaN.  See the module docstring for the semantics."""
    _check_rules(smooth, smooth_mode, merge_gap, min_windows, max_events, activation)
    if isinstance(scores, (list, tuple)):
        scores = np.asarray(scores)
    shape = tuple(scores.shape)
    is_float = scores.dtype.is_floating_point if isinstance(scores, torch.Tensor) else np.asarray(scores).dtype.kind == "f"
    if len(shape) != 2 or shape[1] < 1 or not is_float:
        raise ValueError(f"scores of shape {shape}: a float [M, C] matrix with C >= 1 expected")
    m, n_classes = int(shape[0]), int(shape[1])
    n = m
    rows_host = None
    if row_of_window is not None:
        rshape = tuple(row_of_window.shape) if isinstance(row_of_window, torch.Tensor) else np.asarray(row_of_window).shape
        if len(rshape) != 1:
            raise ValueError(f"row_of_window of shape {rshape}: one row number per window expected")
        n = int(rshape[0])
        if not (isinstance(row_of_window, torch.Tensor) and row_of_window.is_cuda):          # a device list is not read back: the kernel skips rows outside
            rows_host = np.asarray(row_of_window.cpu() if isinstance(row_of_window, torch.Tensor) else row_of_window)
            if rows_host.dtype.kind not in "iu":
                raise ValueError("row_of_window: integers expected")
            if rows_host.size and (int(rows_host.min()) < -1 or int(rows_host.max()) >= m):
                raise ValueError(f"row_of_window outside -1..{m - 1}")
    if windows is not None and windows.n_windows != n:
        raise ValueError(f"windows holds {windows.n_windows} windows, the scores {n}")
    if n > MAX_WINDOWS:
        raise ValueError(f"{n} windows: more than 2^31 - 1 in one call")
    offs = _offsets(seq_offsets, windows, n)
    t_on, t_off = _thresholds(on, off, n_classes, activation)

    _capi.require_gpu()
    lib = _capi.lib()
    st = _as_tensor(scores)
    dev = st.device if st.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        if n == 0 or m == 0:
            return _empty(dev, 0 if max_events is None else int(max_events), activation, windows)
        x = st.to(dev).to(torch.float32)
        if x.stride(1) != 1:
            x = x.contiguous()
        rows = None
        if row_of_window is not None:
            rows = (torch.from_numpy(rows_host.astype(np.int32)) if rows_host is not None else row_of_window).to(dev).to(torch.int32).contiguous()
        off_dev, on_dev, off_thr = _to_device(offs, dev), _to_device(t_on, dev), _to_device(t_off, dev)
        n_seq = len(offs) - 1
        ws_bytes = int(lib.avexhip_events_workspace_bytes(n, n_classes, n_seq))
        if ws_bytes == 0:
            raise _capi.AvexHipError(f"events: no workspace for {n} windows, {n_classes} classes, {n_seq} sequences")
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        total = torch.zeros((), dtype=torch.int64, device=dev)
        a = _capi.EventsArgs()
        a.scores, a.ld_scores, a.n_rows, a.n_windows, a.n_classes, a.n_seq = x.data_ptr(), x.stride(0), m, n, n_classes, n_seq
        a.seq_offsets_host, a.seq_offsets_dev = offs.ctypes.data, off_dev.data_ptr()
        a.row_of_window = rows.data_ptr() if rows is not None else None
        a.on, a.off = on_dev.data_ptr(), off_thr.data_ptr()
        a.smooth, a.smooth_mode, a.merge_gap, a.min_windows = int(smooth), SMOOTH_MODES.index(smooth_mode), int(merge_gap), int(min_windows)
        a.workspace, a.workspace_bytes, a.total = ws.data_ptr(), ws_bytes, total.data_ptr()
        s = _stream()
        _capi.check(lib.avexhip_events_scan(C.byref(a), s), "events_scan")
        cap = int(total.item()) if max_events is None else int(max_events)                   # the one host synchronisation, when asked to size exactly
        out = {name: torch.empty((max(cap, 1),), dtype=dt, device=dev) for name, dt in COLUMNS}
        r = _capi.EventsResult()
        r.capacity = cap
        r.sequence, r.class_id, r.first, r.last = (out[k].data_ptr() for k in ("sequence", "class_id", "first", "last"))
        r.peak, r.peak_window, r.mean = out["peak"].data_ptr(), out["peak_window"].data_ptr(), out["mean"].data_ptr()
        _capi.check(lib.avexhip_events_emit(C.byref(a), C.byref(r), s), "events_emit")
        out = {k: v[:cap] for k, v in out.items()}
        out["count"] = total
        return _derived(out, activation, windows)


def detect_events(model: Any, probe: Callable[[torch.Tensor], torch.Tensor], sources: Sequence[Any], window_s: float, hop_s: Optional[float] = None, *,
                  on=None, off=None, activation: Optional[str] = None, smooth: int = 1, smooth_mode: str = "median", merge_gap: int = 0,
                  min_windows: int = 1, max_events: Optional[int] = None, probe_batch_size: int = 4096, return_scores: bool = False,
                  layers: Optional[Sequence[Any]] = None, aggregation: str = "mean", batch_size: int = 256, min_rms_db: Optional[float] = None,
                  min_peak_db: Optional[float] = None, tail: str = "pad", batch_invariant: Optional[bool] = None, sr: int = 16000,
                  res_type: Optional[str] = None, device: Any = None, max_resident_samples: Optional[int] = None,
                  measure: Optional[Any] = None, activity: Optional[Any] = None) -> Dict[str, Any]:
    """Files to events: the windows of ``sources`` are embedded (:func:`avex_amd.recordings.embed_recordings`, whose gate and model
    arguments this takes), ``probe(emb[lo:hi])`` scores them ``probe_batch_size`` at a time -- any callable from ``[n, D]`` to ``[n, C]``:
    an :mod:`avex_amd.probes` head in ``feature_mode``, or a torch module -- and :func:`decode_events` (whose rule arguments this takes)
    turns the scores into events.  A window the gate dropped has no score: it takes no part in smoothing and clears the state.

    Returns the event dict with ``recording`` / ``start_s`` / ``end_s`` / ``peak_s``, plus ``names`` (the recordings in order: a path
    where the source is one, else its number) and, with ``return_scores``, ``scores [n_kept, C]`` and ``row_of_window [N]``.  With
    ``measure`` (a :class:`avex_amd.measurements.MeasureSpec`) the result gains ``measurements``:
    :func:`avex_amd.measurements.measure_events` of the events over the windows they were decoded with, which the caller never sees."""
    from . import measurements, recordings
    if measure is not None and not isinstance(measure, measurements.MeasureSpec):
        raise TypeError(f"measure: a MeasureSpec expected, not {type(measure).__name__}")
    _check_rules(smooth, smooth_mode, merge_gap, min_windows, max_events, activation)
    _thresholds(on, off, None, activation)
    _int_in(probe_batch_size, 1, 1 << 31, "probe_batch_size")
    if not callable(probe):
        raise ValueError("probe: a callable from [n, D] embeddings to [n, C] scores expected")
    sources = list(sources)
    if len(sources) == 0:
        raise ValueError("no recordings")
    if device is None and isinstance(model, torch.nn.Module):
        p = next(model.parameters(), None)
        device = p.device if p is not None and p.is_cuda else None
    limit = recordings.MAX_RESIDENT_SAMPLES if max_resident_samples is None else max_resident_samples
    ws = recordings._windows_of(sources, window_s, hop_s, sr, tail, res_type, device, limit)
    results = recordings._embed(model, ws, layers, aggregation, batch_size, min_rms_db, min_peak_db, batch_invariant, activity)
    names = [os.fspath(s) if isinstance(s, (str, os.PathLike)) else str(i) for i, s in enumerate(sources)]
    dev = ws.wav.device
    with torch.cuda.device(dev):
        parts = [r["embeddings"] for r in results if not isinstance(r["embeddings"], (list, tuple)) and r["embeddings"].dim() == 2]
        if any(isinstance(r["embeddings"], (list, tuple)) or (r["embeddings"].dim() != 2 and len(r["start_s"])) for r in results):
            raise ValueError("one embedding per window expected (one layer, an aggregation that gives [n, dim])")
        kept = torch.cat([r["kept"] for r in results]).to(dev)
        row_of_window = torch.where(kept, torch.cumsum(kept, 0, dtype=torch.int32) - 1, torch.full((), -1, dtype=torch.int32, device=dev)).to(torch.int32)
        chunks = []
        if parts:
            emb = torch.cat(parts)
            with torch.no_grad():
                for lo in range(0, int(emb.shape[0]), int(probe_batch_size)):
                    chunks.append(probe(emb[lo:lo + int(probe_batch_size)]))
        if chunks:
            scores = torch.cat(chunks)
            if scores.dim() != 2 or scores.shape[0] != emb.shape[0]:
                raise ValueError(f"the probe returned {tuple(scores.shape)} for {tuple(emb.shape)} embeddings: [n, C] expected")
            out = decode_events(scores, windows=ws, on=on, off=off, activation=activation, smooth=smooth, smooth_mode=smooth_mode, merge_gap=merge_gap,
                                min_windows=min_windows, row_of_window=row_of_window, max_events=max_events)
        else:                                         # the gate kept nothing: no score, no event
            scores = torch.empty((0, 0), dtype=torch.float32, device=dev)
            out = _empty(dev, 0 if max_events is None else int(max_events), activation, ws)
        if measure is not None:
            out["measurements"] = measurements.measure_events(out, ws, measure)
    out["names"] = names
    if return_scores:
        out["scores"], out["row_of_window"] = scores, row_of_window
    return out
