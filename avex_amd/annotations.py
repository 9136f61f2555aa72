"""Scoring detections against annotations: which marked calls a decode found, precision / recall / F1 / AP per class, a threshold sweep,
and labelled windows for an :class:`~avex_amd.examples.ExampleBank` out of marked stretches of a recording.

:func:`avex_amd.detection.decode_events` ends at "class c from 12.5 s to 17.0 s of recording r"; this module reads the other side, a Raven
selection table or plain arrays, and compares the two where the events lie.  The overlap of every window with every class and the matching
of predicted with marked events are kernels of ``csrc/annotations.hip``; counts, ratios and the sweep are torch over their outputs.  There
is no CPU fallback: a call without a GPU raises :class:`~avex_amd._capi.AvexHipError` after its arguments are checked.

Semantics (the tests hold them; ``tests/_annotations_ref.py`` restates them in NumPy).  All arithmetic that decides anything is integer
arithmetic on sample counts at ``windows.sr``, or one fp64 multiply and compare.

* **Samples.**  A time ``t`` is sample ``floor(t * sr + 0.5)`` (int64).
* **Reference events.**  Per (recording, class) the annotations sorted by start and merged where they overlap or touch
  (``next.lo <= cur.hi``): two boxes over one stretch are one presence.  An annotation shorter than half a sample covers no sample and
  makes no event.  ``n_ref[c]`` counts the merged ones.  The table is sorted by (recording, class, lo) with one segment per
  (recording, class).
* **Cells.**  Reported as the hull of its windows an event overstates itself by ``(window_len - hop_len) / 2`` on each side when windows
  overlap, and two events of one class one inactive window apart can overlap in time.  Scoring uses cells instead: in recording ``r`` of
  ``n_r`` samples with windows ``0 .. m - 1``, ``c_0 = 0``, ``c_i = clamp(start_i + (window_len - hop_len) // 2, 0, n_r)`` (floor division)
  and ``c_m = n_r``; window ``i`` owns ``[c_i, c_{i+1})`` and an event ``(first, last)`` spans ``[c_first, c_{last+1})``.  Cells partition
  the recording, so the events of one class in one recording are disjoint and ordered.  A cell may be empty (the last windows of a
  ``tail="pad"`` plan); an event of empty cells has length 0 and matches nothing.
* **Overlap** ``[N, C]`` int32: the samples of a window's span -- ``[start, start + valid)`` for ``span="window"``, its cell for
  ``"cell"`` -- that the class-c reference events of its recording cover.
* **Compatible.**  With int64 ``inter`` and ``union`` of a predicted span and a reference event: ``inter > 0`` and
  ``float64(inter) >= iou * float64(union)``, ``1/16 <= iou <= 1``.
* **Matching.**  Per (recording, class) the two-pointer walk over predictions and reference events in time order: compatible -> match
  both and advance both; otherwise advance the one that ends first, the prediction on a tie.  Both sides are disjoint, so compatible
  pairs never cross and the walk is a maximum-cardinality matching.  Matching does not look at scores.
* **Counts.**  ``tp[c]`` matched predictions, ``fp = n_pred - tp``, ``fn = n_ref - tp``; ``precision = tp / n_pred``, ``recall = tp / n_ref``,
  ``f1 = 2 tp / (n_pred + n_ref)``, each one float64 division of integers, NaN where the denominator is 0.  ``micro_*`` from the summed
  counts; ``macro_*`` the mean over the classes with ``n_ref > 0`` (``macro_precision`` over those of them that have a prediction).
* **Average precision.**  Predictions of class c ranked by (peak descending, event number ascending); AP is the sum over matched ranks
  ``k`` of ``tp_cum_k / k``, over ``n_ref[c]``.
"""
from __future__ import annotations

import csv
import ctypes as C
import math
import os
import weakref
from fractions import Fraction
from typing import Any, Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from ._metric_inputs import _stream

__all__ = ["Annotations", "WindowPlan", "window_cells", "window_overlap", "window_labels", "window_classes", "match_events", "score_events",
           "score_windows", "sweep_thresholds", "report", "MIN_IOU", "CHUNK_PAIRS"]

MIN_IOU = 0.0625                          # AVEXHIP_ANNOT_MIN_IOU
CHUNK_PAIRS = 256                         # AVEXHIP_ANNOT_CHUNK_PAIRS
MAX_SPAN = (1 << 31) - 1                  # samples of a span or of a reference event
SPANS = ("window", "cell")
RAVEN_BEGIN, RAVEN_END, RAVEN_SELECTION = "Begin Time (s)", "End Time (s)", "Selection"


class ReferenceEvents(NamedTuple):
    """The merged annotations at one sample rate, sorted by (recording, class, lo)."""
    recording: np.ndarray                 # [A] int32
    class_id: np.ndarray                  # [A] int32
    lo: np.ndarray                        # [A] int64 samples
    hi: np.ndarray                        # [A] int64
    seg_offsets: np.ndarray               # [n_recordings * n_classes + 1] int64: the events of segment r * n_classes + c
    prefix: np.ndarray                    # [A + 1] int64: summed lengths of the events below j
    n_ref: np.ndarray                     # [n_classes] int64


def _ints(x, what: str) -> np.ndarray:
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
    if a.ndim != 1 or (a.dtype.kind not in "iu" and a.size):
        raise ValueError(f"{what}: a 1-d integer array expected")
    return a.astype(np.int64)


class Annotations:
    """Marked calls: parallel 1-d arrays ``recording`` (the index into the ``sources`` of the windows), ``class_id``, ``start_s`` and
    ``end_s`` (seconds, float64).  Refused: NaN or Inf times, ``end_s <= start_s``, a negative start, a negative recording or class, a
    class ``>= n_classes`` (``None``: one more than the largest class given, or ``len(class_names)``).  Immutable."""

    __slots__ = ("recording", "class_id", "start_s", "end_s", "n_classes", "class_names", "_cache", "__weakref__")

    def __init__(self, recording, class_id, start_s, end_s, *, n_classes: Optional[int] = None, class_names: Optional[Sequence[str]] = None) -> None:
        rec, cls = _ints(recording, "recording"), _ints(class_id, "class_id")
        times = []
        for name, x in (("start_s", start_s), ("end_s", end_s)):
            a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
            if a.ndim != 1 or a.dtype.kind not in "iuf":
                raise ValueError(f"{name}: a 1-d array of seconds expected")
            a = a.astype(np.float64)
            if not np.isfinite(a).all():
                raise ValueError(f"{name} holds a NaN or an Inf")
            times.append(a)
        start, end = times
        if not len(rec) == len(cls) == len(start) == len(end):
            raise ValueError(f"recording, class_id, start_s and end_s hold {len(rec)}, {len(cls)}, {len(start)} and {len(end)} entries")
        if (start < 0.0).any():
            raise ValueError(f"annotation {int(np.argmax(start < 0.0))} starts before 0 s")
        if (end <= start).any():
            i = int(np.argmax(end <= start))
            raise ValueError(f"annotation {i}: end_s={end[i]} <= start_s={start[i]}")
        if (rec < 0).any() or (cls < 0).any():
            raise ValueError("a negative recording or class")
        if len(rec) and int(rec.max()) >= 1 << 31:
            raise ValueError("a recording past 2^31 - 1")
        names = None if class_names is None else tuple(str(n) for n in class_names)
        if n_classes is None:
            n_classes = len(names) if names is not None else (int(cls.max()) + 1 if len(cls) else 1)
        if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 1 <= int(n_classes) < 1 << 31:
            raise ValueError(f"n_classes={n_classes!r}: an integer >= 1 expected")
        if names is not None and len(names) != int(n_classes):
            raise ValueError(f"{len(names)} class names for {int(n_classes)} classes")
        if len(cls) and int(cls.max()) >= int(n_classes):
            raise ValueError(f"class {int(cls.max())} with n_classes={int(n_classes)}")
        for a in (rec, cls, start, end):
            a.flags.writeable = False
        for k, v in (("recording", rec), ("class_id", cls), ("start_s", start), ("end_s", end), ("n_classes", int(n_classes)), ("class_names", names), ("_cache", {})):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Annotations is immutable")

    def __delattr__(self, name) -> None:
        raise AttributeError("Annotations is immutable")

    def __len__(self) -> int:
        return len(self.recording)

    @classmethod
    def from_raven(cls, paths: Sequence[Any], *, class_column: str, recording: Optional[Sequence[int]] = None,
                   class_names: Optional[Sequence[str]] = None) -> "Annotations":
        """One tab-separated Raven selection table per recording (``recording=None``: table ``i`` is recording ``i``): the columns
        ``Begin Time (s)``, ``End Time (s)`` and ``class_column``.  Rows of other ``View`` s that repeat a selection count once, keyed by
        the ``Selection`` number.  Classes are numbered in sorted name order unless ``class_names`` fixes them."""
        paths = list(paths)
        recs = list(range(len(paths))) if recording is None else [int(r) for r in recording]
        if len(recs) != len(paths):
            raise ValueError(f"{len(paths)} tables for {len(recs)} recordings")
        rows = []
        for path, r in zip(paths, recs):
            with open(os.fspath(path), newline="", encoding="utf-8-sig") as f:
                reader = csv.DictReader(f, delimiter="\t")
                missing = [c for c in (RAVEN_BEGIN, RAVEN_END, class_column) if c not in (reader.fieldnames or [])]
                if missing:
                    raise ValueError(f"{path}: no column {missing[0]!r}")
                seen = set()
                for n, row in enumerate(reader):
                    key = row.get(RAVEN_SELECTION)
                    if key is not None:
                        if key in seen:
                            continue
                        seen.add(key)
                    try:
                        rows.append((r, str(row[class_column]).strip(), float(row[RAVEN_BEGIN]), float(row[RAVEN_END])))
                    except (TypeError, ValueError) as e:
                        raise ValueError(f"{path}: row {n + 1}: {e}") from e
        names = tuple(sorted({name for _, name, _, _ in rows})) if class_names is None else tuple(str(n) for n in class_names)
        number = {name: i for i, name in enumerate(names)}
        unknown = sorted({name for _, name, _, _ in rows} - set(number))
        if unknown:
            raise ValueError(f"class {unknown[0]!r} is not among class_names")
        return cls(np.asarray([r for r, _, _, _ in rows], dtype=np.int64), np.asarray([number[n] for _, n, _, _ in rows], dtype=np.int64),
                   np.asarray([b for _, _, b, _ in rows], dtype=np.float64), np.asarray([e for _, _, _, e in rows], dtype=np.float64),
                   class_names=names if names else None, n_classes=len(names) if names else 1)

    def to_samples(self, sr: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(lo, hi)`` int64: ``floor(t * sr + 0.5)`` of the starts and the ends."""
        sr = int(sr)
        if sr <= 0:
            raise ValueError(f"sr={sr}")
        return tuple(np.floor(t * float(sr) + 0.5).astype(np.int64) for t in (self.start_s, self.end_s))

    def reference_events(self, sr: int, n_recordings: Optional[int] = None) -> ReferenceEvents:
        """The merged table at ``sr`` for ``n_recordings`` recordings (``None``: as many as the annotations name).  Built once per pair."""
        n_rec = (int(self.recording.max()) + 1 if len(self) else 1) if n_recordings is None else int(n_recordings)
        key = (int(sr), n_rec)
        if key not in self._cache:
            if len(self) and int(self.recording.max()) >= n_rec:
                raise ValueError(f"an annotation of recording {int(self.recording.max())}, the windows hold {n_rec}")
            if n_rec < 1 or n_rec * self.n_classes >= 1 << 31:
                raise ValueError(f"{n_rec} recordings x {self.n_classes} classes")
            lo, hi = self.to_samples(sr)
            keep = hi > lo
            rec, cls, lo, hi = self.recording[keep], self.class_id[keep], lo[keep], hi[keep]
            order = np.lexsort((hi, lo, cls, rec))
            rec, cls, lo, hi = rec[order], cls[order], lo[order], hi[order]
            seg = rec * self.n_classes + cls
            # an annotation opens a new event when its segment is new or it starts past everything before it in the segment
            top = hi.copy()
            new = np.ones(len(seg), dtype=bool)
            if len(seg):
                bound = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
                for a, b in zip(bound, np.r_[bound[1:], len(seg)]):
                    top[a:b] = np.maximum.accumulate(hi[a:b])
                new[1:] = (seg[1:] != seg[:-1]) | (lo[1:] > top[:-1])
            first = np.flatnonzero(new)
            m_lo = lo[first]
            m_hi = np.maximum.reduceat(hi, first) if len(first) else hi[:0]
            m_seg = seg[first]
            if len(m_lo) and int((m_hi - m_lo).max()) > MAX_SPAN:
                raise ValueError(f"a reference event of {int((m_hi - m_lo).max())} samples: more than 2^31 - 1")
            offsets = np.searchsorted(m_seg, np.arange(n_rec * self.n_classes + 1, dtype=np.int64), side="left").astype(np.int64)
            prefix = np.zeros(len(m_lo) + 1, dtype=np.int64)
            np.cumsum(m_hi - m_lo, out=prefix[1:])
            m_cls = (m_seg % self.n_classes).astype(np.int32)
            out = ReferenceEvents((m_seg // self.n_classes).astype(np.int32), m_cls, np.ascontiguousarray(m_lo), np.ascontiguousarray(m_hi), offsets, prefix,
                                  np.bincount(m_cls, minlength=self.n_classes).astype(np.int64))
            for a in out:
                a.flags.writeable = False
            self._cache[key] = out
        return self._cache[key]

    def _on_device(self, sr: int, n_rec: int, dev: torch.device) -> Dict[str, torch.Tensor]:
        key = (int(sr), int(n_rec), str(dev))
        if key not in self._cache:
            ref = self.reference_events(sr, n_rec)
            self._cache[key] = {k: _to_device(np.ascontiguousarray(getattr(ref, k)), dev) for k in ("lo", "hi", "seg_offsets", "prefix", "n_ref", "class_id")}
        return self._cache[key]


class WindowPlan:
    """The host side of a :class:`avex_amd.recordings.RecordingWindows` without a waveform: the sliding windows of recordings of the given
    lengths (samples).  What this module reads of either: ``sr``, ``window_len``, ``hop_len``, ``starts``, ``valids``, ``recording``,
    ``ranges``, ``n_windows`` and the recordings' lengths."""

    def __init__(self, n_samples: Sequence[int], sr: int, window_len: int, hop_len: int, tail: str = "pad") -> None:
        from .recordings import plan_recording_windows
        if len(n_samples) == 0:
            raise ValueError("no recordings")
        self.sr, self.window_len, self.hop_len, self.tail = int(sr), int(window_len), int(hop_len), tail
        self.n_samples = np.asarray([int(n) for n in n_samples], dtype=np.int64)
        plans = [plan_recording_windows(int(n), window_len, hop_len, tail) for n in self.n_samples]
        self.ranges, n = [], 0
        for s, _ in plans:
            self.ranges.append((n, n + len(s)))
            n += len(s)
        if n >= 1 << 31:
            raise ValueError(f"{n} windows: more than 2^31 - 1")
        self.n_windows = n
        self.starts = np.concatenate([s for s, _ in plans])
        self.valids = np.concatenate([v for _, v in plans])
        self.recording = np.concatenate([np.full(len(s), r, dtype=np.int32) for r, (s, _) in enumerate(plans)])
        self.start_s = self.starts.astype(np.float64) / self.sr
        self.end_s = (self.starts + self.valids).astype(np.float64) / self.sr


def _lengths(windows: Any) -> np.ndarray:
    if hasattr(windows, "n_samples"):
        return np.asarray(windows.n_samples, dtype=np.int64)
    return np.asarray([windows._table["n_samples"][w0] for w0, _ in windows.ranges], dtype=np.int64)


def window_cells(windows: Any) -> Tuple[np.ndarray, np.ndarray]:
    """``(lo, hi)`` int64 ``[N]``: the cell of every window (module docstring), from ``windows.starts`` and the recordings' lengths."""
    shift = (int(windows.window_len) - int(windows.hop_len)) // 2          # floor, also when hop > window
    starts = np.asarray(windows.starts, dtype=np.int64)
    lo, hi = np.zeros(len(starts), dtype=np.int64), np.zeros(len(starts), dtype=np.int64)
    for (w0, w1), n in zip(windows.ranges, _lengths(windows)):
        if w1 <= w0:
            continue
        edge = np.clip(starts[w0:w1] + shift, 0, int(n))
        edge[0] = 0
        lo[w0:w1] = edge
        hi[w0:w1 - 1] = edge[1:]
        hi[w1 - 1] = int(n)
    return lo, hi


def _spans(windows: Any, span: str) -> Tuple[np.ndarray, np.ndarray]:
    if span not in SPANS:
        raise ValueError(f"span={span!r}: one of {SPANS} expected")
    if span == "cell":
        lo, hi = window_cells(windows)
    else:
        lo = np.asarray(windows.starts, dtype=np.int64)
        hi = lo + np.asarray(windows.valids, dtype=np.int64)
    if len(lo) and int((hi - lo).max()) > MAX_SPAN:
        raise ValueError(f"a span of {int((hi - lo).max())} samples: more than 2^31 - 1")
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def _to_device(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    """A host array -> the device through pinned memory, without waiting for it."""
    return torch.from_numpy(a if a.flags.writeable else a.copy()).pin_memory().to(dev, non_blocking=True)


_PLANS: "weakref.WeakKeyDictionary[Any, Dict[Any, Any]]" = weakref.WeakKeyDictionary()


def _plan_on(windows: Any, span: str, dev: Optional[torch.device] = None):
    """The host spans ``(lo, hi)`` of the windows, made once per (windows, span); with ``dev`` their device copies, uploaded once."""
    per = _PLANS.setdefault(windows, {})
    if span not in per:
        per[span] = _spans(windows, span)
    if dev is None:
        return per[span]
    key = (span, str(dev))
    if key not in per:
        per[key] = tuple(_to_device(a, dev) for a in per[span])
    return per[key]


def _check_pair(windows: Any, annotations: Any) -> None:
    if not isinstance(annotations, Annotations):
        raise TypeError(f"an Annotations expected, not {type(annotations).__name__}")
    for name in ("sr", "window_len", "hop_len", "starts", "valids", "recording", "ranges", "n_windows"):
        if not hasattr(windows, name):
            raise TypeError(f"windows: a RecordingWindows or a WindowPlan expected ({type(windows).__name__} has no {name!r})")


def _device(windows: Any, *tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    wav = getattr(windows, "wav", None)
    return wav.device if isinstance(wav, torch.Tensor) and wav.is_cuda else torch.device("cuda", torch.cuda.current_device())


def window_overlap(windows: Any, annotations: Annotations, *, span: str = "window") -> torch.Tensor:
    """int32 ``[N, C]`` on the device: the samples of every window's span that the class-c reference events of its recording cover.
    ``span="window"``: ``[start, start + valid)``; ``"cell"``: the window's cell.  One launch, no host synchronisation."""
    _check_pair(windows, annotations)
    _plan_on(windows, span)                               # refuses an unknown span and spans past 2^31 - 1 samples
    n, n_rec, n_cls = int(windows.n_windows), len(windows.ranges), annotations.n_classes
    ref = annotations.reference_events(windows.sr, n_rec)
    _capi.require_gpu()
    dev = _device(windows)
    with torch.cuda.device(dev):
        out = torch.zeros((n, n_cls), dtype=torch.int32, device=dev)
        if n == 0 or len(ref.lo) == 0:
            return out
        lo_dev, hi_dev = _plan_on(windows, span, dev)
        t = annotations._on_device(windows.sr, n_rec, dev)
        win_rec = np.ascontiguousarray(windows.recording, dtype=np.int32)
        win_rec_dev = _to_device(win_rec, dev)
        _capi.check(_capi.lib().avexhip_annot_overlap(lo_dev.data_ptr(), hi_dev.data_ptr(), win_rec.ctypes.data, win_rec_dev.data_ptr(), n, n_rec, n_cls,
                                                      ref.seg_offsets.ctypes.data, t["seg_offsets"].data_ptr(), t["lo"].data_ptr(), t["hi"].data_ptr(),
                                                      t["prefix"].data_ptr(), len(ref.lo), out.data_ptr(), _stream()), "annot_overlap")
    return out


def _label_rules(sr: int, min_overlap_s, min_fraction) -> Tuple[int, Optional[Fraction]]:
    need = 1
    if min_overlap_s is not None:
        if isinstance(min_overlap_s, bool) or not isinstance(min_overlap_s, (int, float, np.integer, np.floating)) or not math.isfinite(float(min_overlap_s)) \
                or float(min_overlap_s) < 0.0:
            raise ValueError(f"min_overlap_s={min_overlap_s!r}: a number of seconds >= 0 expected")
        need = max(1, int(math.floor(float(min_overlap_s) * sr + 0.5)))
    frac = None
    if min_fraction is not None:
        if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, np.integer, np.floating, Fraction)) \
                or not (isinstance(min_fraction, Fraction) or math.isfinite(float(min_fraction))) or not 0 < min_fraction <= 1:
            raise ValueError(f"min_fraction={min_fraction!r}: a number in (0, 1] expected")
        frac = Fraction(min_fraction).limit_denominator(1000)
        if frac <= 0:
            raise ValueError(f"min_fraction={min_fraction!r} is below 1/1000")
    return need, frac


def window_labels(windows: Any, annotations: Annotations, *, span: str = "window", min_overlap_s: Optional[float] = None,
                  min_fraction: Optional[float] = None) -> torch.Tensor:
    """bool ``[N, C]`` on the device: ``overlap >= max(1, floor(min_overlap_s * sr + 0.5))`` and, with ``min_fraction`` (taken as
    ``Fraction(min_fraction).limit_denominator(1000) = num / den``), ``overlap * den >= num * span_len`` in int64.  With neither: one
    sample of overlap labels a window."""
    _check_pair(windows, annotations)
    need, frac = _label_rules(int(windows.sr), min_overlap_s, min_fraction)
    ov = window_overlap(windows, annotations, span=span)
    labels = ov >= need
    if frac is not None and ov.shape[0]:
        lo_dev, hi_dev = _plan_on(windows, span, ov.device)
        labels &= ov.long() * frac.denominator >= frac.numerator * (hi_dev - lo_dev)[:, None]
    return labels


def window_classes(windows: Any, annotations: Annotations, *, span: str = "window", min_overlap_s: Optional[float] = None,
                   min_fraction: Optional[float] = None) -> torch.Tensor:
    """int32 ``[N]`` on the device: the class of a window that exactly one class labels, ``-1`` where none does (the background label of
    :class:`~avex_amd.examples.ExampleBank`), ``-2`` where several do."""
    labels = window_labels(windows, annotations, span=span, min_overlap_s=min_overlap_s, min_fraction=min_fraction)
    count = labels.sum(dim=1)
    cls = labels.to(torch.int32).argmax(dim=1).to(torch.int32)
    return torch.where(count == 1, cls, torch.where(count == 0, torch.full_like(cls, -1), torch.full_like(cls, -2)))


def _check_iou(iou) -> float:
    if isinstance(iou, bool) or not isinstance(iou, (int, float, np.integer, np.floating)) or not MIN_IOU <= float(iou) <= 1.0:
        raise ValueError(f"iou={iou!r}: a number in [{MIN_IOU}, 1] expected")
    return float(iou)


def _pred_columns(pred: Any) -> Dict[str, torch.Tensor]:
    if not isinstance(pred, dict) or any(k not in pred for k in ("sequence", "class_id", "first", "last")):
        raise ValueError("pred: the dict decode_events returns expected (sequence, class_id, first, last)")
    cols = {k: pred[k] for k in ("sequence", "class_id", "first", "last")}
    shape = None
    for k, t in cols.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"pred[{k!r}]: an int32 1-d tensor expected")
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"pred[{k!r}] holds {tuple(t.shape)[0]} rows, the other columns {shape[0]}")
        shape = tuple(t.shape)
    if shape[0] >= (1 << 31) - CHUNK_PAIRS:
        raise ValueError(f"{shape[0]} predictions: more than one call takes")
    return cols


def match_events(pred: Dict[str, torch.Tensor], annotations: Annotations, windows: Any, *, iou: float = 0.5) -> Dict[str, torch.Tensor]:
    """Match the events of a :func:`~avex_amd.detection.decode_events` dict with the reference events (module docstring), on the device.

    Returns ``match_of_pred [P]`` (int32: the reference event of each row of ``pred``, ``-1`` for none and for filler rows),
    ``match_of_ref [A]`` (the row matched with each reference event, numbered as in ``annotations.reference_events``), ``pred_lo`` /
    ``pred_hi`` (int64 ``[P]``: the predicted spans in samples, 0 for filler rows) and ``order_errors`` (int64 scalar: rows that are
    malformed or out of the decode order, plus one when pairs had to be dropped; when it is nonzero the other outputs are unspecified).
    Nothing is read back."""
    _check_pair(windows, annotations)
    iou = _check_iou(iou)
    cols = _pred_columns(pred)
    n, n_rec, n_cls = int(windows.n_windows), len(windows.ranges), annotations.n_classes
    ref = annotations.reference_events(windows.sr, n_rec)
    _plan_on(windows, "cell")
    n_pred, n_ref = int(cols["first"].shape[0]), len(ref.lo)
    if n_pred + n_ref >= (1 << 31) - CHUNK_PAIRS:
        raise ValueError(f"{n_pred} predictions and {n_ref} reference events: more than one call takes")
    _capi.require_gpu()
    lib = _capi.lib()
    dev = _device(windows, cols["first"])
    with torch.cuda.device(dev):
        cols = {k: t.to(dev).contiguous() for k, t in cols.items()}
        mop = torch.full((n_pred,), -1, dtype=torch.int32, device=dev)
        mor = torch.full((n_ref,), -1, dtype=torch.int32, device=dev)
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        if n == 0 or n_pred == 0:
            return {"match_of_pred": mop, "match_of_ref": mor, "pred_lo": torch.zeros(n_pred, dtype=torch.int64, device=dev),
                    "pred_hi": torch.zeros(n_pred, dtype=torch.int64, device=dev), "order_errors": zero}
        lo_dev, hi_dev = _plan_on(windows, "cell", dev)
        valid = (cols["first"] >= 0) & (cols["last"] >= cols["first"]) & (cols["last"] < n)
        pred_lo = torch.where(valid, lo_dev[cols["first"].clamp(0, n - 1).long()], zero)
        pred_hi = torch.where(valid, hi_dev[cols["last"].clamp(0, n - 1).long()], zero)
        out = {"match_of_pred": mop, "match_of_ref": mor, "pred_lo": pred_lo, "pred_hi": pred_hi}
        if n_ref == 0:                                   # nothing to match with; the rows are still checked for their ranges
            bad = (cols["first"] >= 0) & ~(valid & (cols["sequence"] >= 0) & (cols["sequence"] < n_rec) & (cols["class_id"] >= 0) & (cols["class_id"] < n_cls))
            out["order_errors"] = bad.sum(dtype=torch.int64)
            return out
        t = annotations._on_device(windows.sr, n_rec, dev)
        ws_bytes = int(lib.avexhip_annot_workspace_bytes(n_pred, n_ref, n_rec * n_cls))
        if ws_bytes == 0:
            raise _capi.AvexHipError(f"annotations: no workspace for {n_pred} predictions, {n_ref} reference events, {n_rec * n_cls} segments")
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        counts = torch.empty((n_pred,), dtype=torch.int64, device=dev)
        errors = torch.empty((n_pred,), dtype=torch.int32, device=dev)
        a = _capi.AnnotMatchArgs()
        a.sequence, a.class_id, a.first, a.last = (cols[k].data_ptr() for k in ("sequence", "class_id", "first", "last"))
        a.n_pred, a.n_windows, a.n_ref, a.n_rec, a.n_classes, a.iou = n_pred, n, n_ref, n_rec, n_cls, iou
        a.cell_lo, a.cell_hi = lo_dev.data_ptr(), hi_dev.data_ptr()
        a.seg_offsets_host, a.seg_offsets_dev = ref.seg_offsets.ctypes.data, t["seg_offsets"].data_ptr()
        a.ref_lo, a.ref_hi = t["lo"].data_ptr(), t["hi"].data_ptr()
        a.workspace, a.workspace_bytes, a.counts, a.errors = ws.data_ptr(), ws_bytes, counts.data_ptr(), errors.data_ptr()
        s = _stream()
        _capi.check(lib.avexhip_annot_count(C.byref(a), s), "annot_count")
        offsets = torch.zeros((n_pred + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        _capi.check(lib.avexhip_annot_match(C.byref(a), offsets.data_ptr(), mop.data_ptr(), mor.data_ptr(), s), "annot_match")
        out["order_errors"] = errors.sum(dtype=torch.int64) + (offsets[n_pred] > n_pred + n_ref).to(torch.int64)
        return out


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """One float64 division of integers; NaN where the denominator is 0."""
    d = den.to(torch.float64)
    return torch.where(den != 0, num.to(torch.float64) / torch.where(den != 0, d, torch.ones_like(d)), torch.full_like(d, math.nan))


def _aggregates(out: Dict[str, torch.Tensor], tp, n_pred, n_ref) -> None:
    out["precision"], out["recall"], out["f1"] = _ratio(tp, n_pred), _ratio(tp, n_ref), _ratio(2 * tp, n_pred + n_ref)
    stp, sp, sr_ = tp.sum(), n_pred.sum(), n_ref.sum()
    out["micro_precision"], out["micro_recall"], out["micro_f1"] = _ratio(stp, sp), _ratio(stp, sr_), _ratio(2 * stp, sp + sr_)
    has = n_ref > 0
    zero = torch.zeros((), dtype=torch.float64, device=tp.device)
    for name, mask in (("precision", has & (n_pred > 0)), ("recall", has), ("f1", has)):
        mean = torch.where(mask, out[name], zero).sum() / mask.sum().clamp(min=1).to(torch.float64)
        out["macro_" + name] = torch.where(mask.any(), mean, zero + math.nan)


_SUM_BLOCK = 4096


def _class_sums(term: torch.Tensor, bucket: torch.Tensor, local: torch.Tensor, n_per: torch.Tensor) -> torch.Tensor:
    """float64 ``[n_buckets]``: the sum of ``term`` per bucket, for rows sorted by bucket (``local``: a row's place inside its bucket,
    ``n_per``: the rows of every bucket).  Two dense passes -- rows into blocks of 4096 of ONE bucket, blocks into their bucket's row --
    summed along an axis: no atomics, so one bucket of 10^6 rows costs what 10^3 buckets of 10^3 do, and the bits are the same on every run."""
    n_rows, n_buckets, dev = int(term.shape[0]), int(n_per.shape[0]), term.device
    per_bucket = n_rows // _SUM_BLOCK + 1                                                 # blocks one bucket can have at most
    blocks = (n_per + _SUM_BLOCK - 1) // _SUM_BLOCK
    n_blocks = n_rows // _SUM_BLOCK + n_buckets                                           # >= the sum of ceil(n / 4096)
    block = (torch.cumsum(blocks, 0) - blocks)[bucket] + local // _SUM_BLOCK
    dense = torch.zeros(n_blocks * _SUM_BLOCK, dtype=torch.float64, device=dev)
    dense[block * _SUM_BLOCK + local % _SUM_BLOCK] = term                                 # every row has a slot of its own
    partial = dense.view(n_blocks, _SUM_BLOCK).sum(1)
    slot = torch.full((n_blocks,), n_buckets * per_bucket, dtype=torch.int64, device=dev)  # blocks no row falls into go to a spare slot, as 0
    slot[block] = bucket * per_bucket + local // _SUM_BLOCK                               # (the rows of a block all write the same number)
    rows = torch.zeros(n_buckets * per_bucket + 1, dtype=torch.float64, device=dev)
    rows[slot] = partial
    return rows[:n_buckets * per_bucket].view(n_buckets, per_bucket).sum(1)


def score_events(pred: Dict[str, torch.Tensor], annotations: Annotations, windows: Any, *, iou: float = 0.5) -> Dict[str, torch.Tensor]:
    """Event-level scores of a :func:`~avex_amd.detection.decode_events` dict against ``annotations``, as device tensors without a host
    synchronisation: per class int64 ``n_pred``, ``n_ref``, ``tp``, ``fp``, ``fn`` and float64 ``precision``, ``recall``, ``f1``,
    ``average_precision`` (ranked by ``pred["peak"]``; NaN for a class without a reference event); ``micro_*`` / ``macro_*`` scalars;
    ``match_of_pred``, ``match_of_ref``, ``iou_of_pred`` (float64 ``inter / union``, NaN when unmatched) and ``order_errors``.
    :func:`report` copies a result to the host."""
    m = match_events(pred, annotations, windows, iou=iou)
    n_cls = annotations.n_classes
    dev = m["match_of_pred"].device
    with torch.cuda.device(dev):
        first, cls = pred["first"].to(dev), pred["class_id"].to(dev)
        n_rows = int(first.shape[0])
        valid = (first >= 0) & (cls >= 0) & (cls < n_cls)
        bucket = torch.where(valid, cls, torch.full_like(cls, n_cls)).long()            # filler rows fall into bucket C
        matched = valid & (m["match_of_pred"] >= 0)
        # Ranks: a stable sort by peak descending, then a stable sort by class, leaves every class's rows together in (peak descending,
        # row ascending) order.  Counts are then differences of integer prefixes at the class edges -- no scatter onto one address per class.
        peak = pred["peak"].to(dev).to(torch.float64) if "peak" in pred else torch.zeros(n_rows, dtype=torch.float64, device=dev)
        by_peak = torch.sort(-peak, stable=True).indices
        by_class = torch.sort(bucket[by_peak], stable=True)
        order, b = by_peak[by_class.indices], by_class.values
        edges = torch.searchsorted(b, torch.arange(n_cls + 2, dtype=torch.int64, device=dev))          # rows of the buckets below c
        per = edges[1:] - edges[:-1]
        hit = matched[order].long()
        cum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(hit, 0)])         # hits among the first x rows
        n_pred, tp = per[:n_cls], (cum[edges[1:]] - cum[edges[:-1]])[:n_cls]
        n_ref = annotations._on_device(windows.sr, len(windows.ranges), dev)["n_ref"] if m["match_of_ref"].numel() else torch.zeros(n_cls, dtype=torch.int64, device=dev)
        out: Dict[str, torch.Tensor] = {"n_pred": n_pred, "n_ref": n_ref, "tp": tp, "fp": n_pred - tp, "fn": n_ref - tp}
        _aggregates(out, tp, n_pred, n_ref)
        out.update(match_of_pred=m["match_of_pred"], match_of_ref=m["match_of_ref"], order_errors=m["order_errors"])
        nan = torch.full((), math.nan, dtype=torch.float64, device=dev)
        if m["match_of_ref"].numel():
            t = annotations._on_device(windows.sr, len(windows.ranges), dev)
            j = m["match_of_pred"].clamp(min=0).long()
            inter = torch.minimum(m["pred_hi"], t["hi"][j]) - torch.maximum(m["pred_lo"], t["lo"][j])
            union = torch.maximum(m["pred_hi"], t["hi"][j]) - torch.minimum(m["pred_lo"], t["lo"][j])
            out["iou_of_pred"] = torch.where(matched & (union > 0), inter.to(torch.float64) / union.clamp(min=1).to(torch.float64), nan)
        else:
            out["iou_of_pred"] = nan.expand(n_rows).clone()
        start = edges[b]                                                                # rows in front of the row's class
        local = torch.arange(n_rows, dtype=torch.int64, device=dev) - start
        prec_at = (cum[1:] - cum[start]).to(torch.float64) / (local + 1).to(torch.float64)             # tp_cum_k / k at rank k = local + 1
        ap = _class_sums(torch.where(hit > 0, prec_at, torch.zeros_like(prec_at)), b, local, per)
        out["average_precision"] = torch.where(n_ref > 0, ap[:n_cls] / n_ref.clamp(min=1).to(torch.float64), nan)
        return out


def score_windows(pred: Dict[str, torch.Tensor], annotations: Annotations, windows: Any, *, min_overlap_s: Optional[float] = None,
                  min_fraction: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """The window-level counterpart of :func:`score_events`: the events rasterised to bool ``[N, C]`` (a difference array and an integer
    cumsum) against ``window_labels(span="cell")``.  Per class int64 ``tp``, ``fp``, ``fn``, ``tn`` and float64 ``precision``, ``recall``,
    ``f1``, with the ``micro_*`` / ``macro_*`` scalars; ``predicted`` and ``labels`` are the two matrices.  No host synchronisation."""
    _check_pair(windows, annotations)
    cols = _pred_columns(pred)
    labels = window_labels(windows, annotations, span="cell", min_overlap_s=min_overlap_s, min_fraction=min_fraction)
    n, n_cls, dev = int(windows.n_windows), annotations.n_classes, labels.device
    with torch.cuda.device(dev):
        first, last, cls = (cols[k].to(dev).long() for k in ("first", "last", "class_id"))
        valid = (first >= 0) & (last >= first) & (last < n) & (cls >= 0) & (cls < n_cls)
        step = torch.zeros((n + 1) * n_cls + first.shape[0], dtype=torch.int32, device=dev)
        sink = (n + 1) * n_cls + torch.arange(first.shape[0], dtype=torch.int64, device=dev)           # a row that is no event adds 0 to an entry of its own
        step.scatter_add_(0, torch.where(valid, first * n_cls + cls, sink), valid.to(torch.int32))
        step.scatter_add_(0, torch.where(valid, (last + 1) * n_cls + cls, sink), -valid.to(torch.int32))
        predicted = torch.cumsum(step[:(n + 1) * n_cls].view(n + 1, n_cls), 0)[:n] > 0
        tp, fp, fn = ((a & b).sum(0, dtype=torch.int64) for a, b in ((predicted, labels), (predicted, ~labels), (~predicted, labels)))
        out: Dict[str, torch.Tensor] = {"tp": tp, "fp": fp, "fn": fn, "tn": (~predicted & ~labels).sum(0, dtype=torch.int64), "n_pred": tp + fp, "n_ref": tp + fn}
        _aggregates(out, tp, tp + fp, tp + fn)
        out.update(predicted=predicted, labels=labels)
        return out


STACKED = ("n_pred", "n_ref", "tp", "fp", "fn", "precision", "recall", "f1", "average_precision")


def sweep_thresholds(scores, windows: Any, annotations: Annotations, thresholds, *, off_ratio: float = 1.0, iou: float = 0.5, row_of_window=None,
                     **rules) -> Dict[str, torch.Tensor]:
    """``decode_events(scores, windows=windows, on=t, off=t * off_ratio, row_of_window=..., **rules)`` and :func:`score_events` for each
    ``t`` of ``thresholds`` (``rules``: ``activation``, ``smooth``, ``smooth_mode``, ``merge_gap``, ``min_windows``, ``max_events``).

    Returns ``thresholds [T]`` (float64), the counts and ratios stacked to ``[T, C]``, ``micro_*`` / ``macro_*`` ``[T]``, ``order_errors``
    (their sum) and ``best_threshold [C]``: the threshold of the highest F1 -- NaN never wins, ties go to the lowest threshold, a class
    whose F1 is NaN throughout gets NaN.  The only host synchronisation is ``decode_events``' own sizing read; none with ``max_events``."""
    from .detection import decode_events
    _check_pair(windows, annotations)
    iou = _check_iou(iou)
    th = np.asarray(thresholds, dtype=np.float64)
    if th.ndim != 1 or th.size == 0 or not np.isfinite(th).all():
        raise ValueError("thresholds: a non-empty 1-d array of finite numbers expected")
    if isinstance(off_ratio, bool) or not isinstance(off_ratio, (int, float, np.integer, np.floating)) or not 0.0 < float(off_ratio) <= 1.0:
        raise ValueError(f"off_ratio={off_ratio!r}: a number in (0, 1] expected")
    for k in ("on", "off", "windows", "seq_offsets"):
        if k in rules:
            raise TypeError(f"sweep_thresholds() sets {k!r} itself")
    runs = []
    for t in th:
        pred = decode_events(scores, windows=windows, on=float(t), off=float(t) * float(off_ratio), row_of_window=row_of_window, **rules)
        runs.append(score_events(pred, annotations, windows, iou=iou))
    dev = runs[0]["tp"].device
    with torch.cuda.device(dev):
        out = {k: torch.stack([r[k] for r in runs]) for k in STACKED + tuple(p + n for p in ("micro_", "macro_") for n in ("precision", "recall", "f1"))}
        out["order_errors"] = torch.stack([r["order_errors"] for r in runs]).sum()
        out["thresholds"] = torch.from_numpy(th).to(dev)
        f1 = out["f1"]
        order = torch.from_numpy(np.argsort(th, kind="stable")).to(dev)                    # argmax returns the first maximum: look in threshold order
        key = torch.where(torch.isnan(f1), torch.full_like(f1, -1.0), f1)[order]
        best = order[key.argmax(dim=0)]
        out["best_threshold"] = torch.where(key.max(dim=0).values >= 0, out["thresholds"][best], torch.full((), math.nan, dtype=torch.float64, device=dev))
        return out


def report(result: Dict[str, torch.Tensor], class_names: Optional[Sequence[str]] = None) -> Dict[str, Any]:
    """The one function here that copies to the host: a result of :func:`score_events`, :func:`score_windows` or :func:`sweep_thresholds`
    as NumPy arrays and Python numbers, with ``per_class`` rows named by ``class_names`` for the first two.  Raises
    :class:`~avex_amd._capi.AvexHipError` when ``order_errors != 0``: the predictions were not a decode's, and the numbers mean nothing."""
    host = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in result.items()}
    if "order_errors" in host and int(host["order_errors"]) != 0:
        raise _capi.AvexHipError(f"annotations: {int(host['order_errors'])} predictions are malformed or out of the decode order "
                                 "(sequence, class, first); scores of such input are not defined")
    out = {k: (v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v) for k, v in host.items()}
    if "tp" in host and host["tp"].ndim == 1:
        names = [str(i) for i in range(len(host["tp"]))] if class_names is None else [str(n) for n in class_names]
        if len(names) != len(host["tp"]):
            raise ValueError(f"{len(names)} class names for {len(host['tp'])} classes")
        keys = [k for k in STACKED + ("tn",) if k in host]
        out["per_class"] = {n: {k: host[k][c].item() for k in keys} for c, n in enumerate(names)}
    return out
