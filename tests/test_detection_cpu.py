"""avex_amd.detection without a GPU: the NumPy restatement against hand-written cases, the ABI 16 bindings and struct layouts, the
workspace size, the refusals of the entry points, and every ValueError of the Python layer."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _detection_ref as D
from avex_amd import _capi, detection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMS = ("avexhip_events_max_smooth", "avexhip_events_max_span", "avexhip_events_chunk_windows", "avexhip_events_workspace_bytes", "avexhip_events_scan",
        "avexhip_events_emit")
NAN = np.nan


def _col(*values):
    return np.asarray(values, dtype=np.float32)[:, None]


def _spans(ev):
    return list(zip(ev["first"].tolist(), ev["last"].tolist()))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_the_worked_example():
    x = _col(2, .5, .5, NAN, .5, 2, -1, 2)
    st = {}
    ev = D.decode(x, [0, 8], 1.0, 0.0, stats=st)
    assert _spans(ev) == [(0, 2), (5, 5), (7, 7)] and st["raw"] == 3                      # the NaN clears: window 4 holds an inactive state
    assert ev["peak"].tolist() == [2.0, 2.0, 2.0] and ev["peak_window"].tolist() == [0, 5, 7] and ev["mean"].tolist() == [1.0, 2.0, 2.0]
    assert ev["sequence"].tolist() == [0, 0, 0] and ev["class_id"].tolist() == [0, 0, 0]
    assert ev["peak"].dtype == np.float32 and ev["mean"].dtype == np.float64 and ev["first"].dtype == np.int32
    ev = D.decode(x, [0, 8], 1.0, 0.0, merge_gap=1, stats=st)
    assert _spans(ev) == [(0, 2), (5, 7)] and (st["raw"], st["merged"], st["kept"]) == (3, 2, 2)
    assert ev["mean"].tolist() == [1.0, 1.0] and ev["peak_window"].tolist() == [0, 5]       # (2 - 1 + 2) / 3; the tie goes to the lower window
    assert _spans(D.decode(x, [0, 8], 1.0, 0.0, merge_gap=1, min_windows=2)) == [(0, 2), (5, 7)]
    assert _spans(D.decode(x, [0, 8], 1.0, 0.0, merge_gap=1, min_windows=4)) == []
    assert _spans(D.decode(x, [0, 8], 1.0, 0.0, min_windows=2)) == [(0, 2)]                # dropped after merging, not before
    assert _spans(D.decode(x, [0, 8], 1.0, 0.0, merge_gap=2)) == [(0, 7)]                  # windows 3 and 4 are a gap of two


def test_holds_never_start_and_sets_do_not_leak():
    assert _spans(D.decode(_col(.5, .5, .9, .5), [0, 4], 1.0, 0.0)) == []                  # all hold: no event
    x = _col(0.5, 2, .5, .5, 2)                                                             # a set in the last window of sequence 0 ...
    ev = D.decode(x, [0, 2, 5], 1.0, 0.0)
    assert _spans(ev) == [(1, 1), (4, 4)] and ev["sequence"].tolist() == [0, 1]             # ... does not make the holds of sequence 1 active
    assert _spans(D.decode(x, [0, 5], 1.0, 0.0)) == [(1, 4)]                                # in one sequence it does
    assert _spans(D.decode(x, [0, 2, 5], 1.0, 0.0, merge_gap=4)) == [(1, 1), (4, 4)]        # and no gap is merged across the boundary
    assert _spans(D.decode(x, [0, 0, 2, 2, 5, 5], 1.0, 0.0)) == [(1, 1), (4, 4)]            # empty sequences change the numbers only
    assert D.decode(x, [0, 0, 2, 2, 5, 5], 1.0, 0.0)["sequence"].tolist() == [1, 3]


def test_smoothing_edges_and_ties():
    x = np.asarray([4, 1, 3, NAN, 2], dtype=np.float32)
    assert D.smooth_sequence(x, 1, "median").tolist()[:3] == [4, 1, 3]
    med = D.smooth_sequence(x, 3, "median")
    assert med.tolist() == [1, 3, 1, 2, 2]                 # the lower median: of (4, 1) -> 1 at the edge, of (1, 3) -> 1, of (3, 2) -> 2
    mean = D.smooth_sequence(x, 3, "mean")
    assert mean.tolist() == [2.5, np.float32(8) / np.float32(3), 2.0, 2.5, 2.0] and mean.dtype == np.float32
    assert np.isnan(D.smooth_sequence(np.asarray([NAN, NAN, 1], dtype=np.float32), 3, "median")[0])
    assert D.smooth_sequence(np.asarray([NAN, NAN, 1], dtype=np.float32), 5, "mean").tolist() == [1, 1, 1]
    ev = D.decode(_col(1, 3, 3, 2), [0, 4], 1.0)                                             # peak ties: the lowest window
    assert ev["peak"].tolist() == [3.0] and ev["peak_window"].tolist() == [1] and ev["mean"].tolist() == [2.25]
    ev = D.decode(_col(1, .5, 1, .99), [0, 4], 1.0)                                          # off == on: no hold band at all
    assert _spans(ev) == [(0, 0), (2, 2)]
    both = np.stack([np.asarray([2, 0, 2, 0], dtype=np.float32), np.asarray([0, 2, 2, 0], dtype=np.float32)], axis=1)
    ev = D.decode(both, [0, 2, 4], [1.0, 1.0], [0.5, 0.5])                                   # the order: sequence, then class, then first
    assert list(zip(ev["sequence"].tolist(), ev["class_id"].tolist(), ev["first"].tolist())) == [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 2)]


# ------------------------------------------------------------------------------------------------------------------ the bindings
def test_bindings_and_limits(built_lib):
    assert _capi.header_abi_version() >= 16
    for name in SYMS:
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name
    hdr = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/avexhip.h").read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(avexhip_events_[a-z0-9_]+)\s*\(", hdr))) == sorted(SYMS)
    assert built_lib.avexhip_events_max_smooth() == 31 == detection.MAX_SMOOTH
    assert built_lib.avexhip_events_max_span() == 64 == detection.MAX_SPAN
    k = built_lib.avexhip_events_chunk_windows()
    assert k >= 64 and k % 64 == 0


def test_events_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the ABI 16 structs as gcc sees include/avexhip.h == the ctypes mirrors."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = {"avexhip_events_args": _capi.EventsArgs, "avexhip_events_result": _capi.EventsResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/avexhip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_workspace_is_monotone_bounded_and_refuses_bad_shapes(built_lib):
    ws = built_lib.avexhip_events_workspace_bytes
    k = built_lib.avexhip_events_chunk_windows()
    base = (100000, 40, 7)
    for axis, steps in enumerate(((1, k - 1, k, k + 1, 100000, 1 << 20, (1 << 31) - 1), (1, 2, 15, 16, 17, 40, 1000), (1, 2, 7, 512, 100000))):
        sizes = []
        for v in steps:
            a = list(base)
            a[axis] = v
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (axis, sizes)
    # at most N * C bytes plus a fixed number of 8-byte words per (chunk, class) and per (sequence, class): four words of window bits,
    # two 32-byte partials and the counts per (chunk, class) make 14; one word per (sequence boundary, class) and one per boundary
    for n, c, r in (base, (1, 1, 1), (k, 1, 1), (k + 1, 3, 2), (1 << 20, 1, 1), (1 << 18, 64, 3), (1 << 16, 1024, 1), (1 << 20, 32, 512), (40, 65, 40)):
        chunks = (n + k - 1) // k
        assert 0 < ws(n, c, r) <= n * c + 8 * (14 * (chunks + 1) * c + 2 * (r + 1) * (c + 1)) + 16 * 11, (n, c, r)
    for bad in ((0, 4, 1), (-1, 4, 1), (1 << 31, 4, 1), (100, 0, 1), (100, -2, 1), (100, 4, 0), (100, 4, -1), ((1 << 31) - 1, 1 << 20, 1)):
        assert ws(*bad) == 0, bad


_KEEP = []


def _args(n=8, c=2, offsets=(0, 3, 8), **kw):
    fake = 1 << 20                                                        # never dereferenced: the call is refused first
    off = np.asarray(offsets, dtype=np.int64)
    _KEEP.append(off)
    a = _capi.EventsArgs()
    a.scores, a.ld_scores, a.n_rows, a.n_windows, a.n_classes, a.n_seq = fake, c, n, n, c, len(off) - 1
    a.seq_offsets_host, a.seq_offsets_dev, a.on, a.off = off.ctypes.data, fake, fake, fake
    a.smooth, a.smooth_mode, a.merge_gap, a.min_windows = 1, 0, 0, 1
    a.workspace, a.workspace_bytes, a.total = fake, 1 << 30, fake
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _result(**kw):
    r = _capi.EventsResult()
    r.capacity = 4
    for name in ("sequence", "class_id", "first", "last", "peak", "peak_window", "mean"):
        setattr(r, name, 1 << 20)
    for key, v in kw.items():
        setattr(r, key, v)
    return r


def test_entry_points_refuse_bad_arguments(built_lib):
    """rc -1 and a message that names the offending number, before the device is touched."""
    lib = built_lib
    calls = ((lambda a: lib.avexhip_events_scan(C.byref(a), None), "events_scan"),
             (lambda a: lib.avexhip_events_emit(C.byref(a), C.byref(_result()), None), "events_emit"))

    def refused(rc, *words):
        msg = _capi.last_error()
        assert rc == -1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    for fn, name in calls:
        for field in ("scores", "seq_offsets_host", "seq_offsets_dev", "on", "off", "workspace", "total"):
            refused(fn(_args(**{field: None})), name, "null")
        refused(fn(_args(n=1 << 31, offsets=(0, 1 << 31))), name, "n_windows 2147483648")
        refused(fn(_args(n=0, offsets=(0, 0))), "n_windows 0")
        refused(fn(_args(n_classes=0)), "n_classes 0")
        refused(fn(_args(n_seq=0)), "n_seq 0")
        refused(fn(_args(ld_scores=1)), "ld_scores 1")
        refused(fn(_args(n_rows=5)), "n_rows 5", "row_of_window")
        refused(fn(_args(n_rows=0, row_of_window=1 << 20)), "n_rows 0")
        for bad in (0, 2, 4, 30, 33, -1):
            refused(fn(_args(smooth=bad)), f"smooth {bad}")
        refused(fn(_args(smooth_mode=2)), "smooth_mode 2")
        for bad in (-1, 65):
            refused(fn(_args(merge_gap=bad)), f"merge_gap {bad}")
        for bad in (0, 65, -3):
            refused(fn(_args(min_windows=bad)), f"min_windows {bad}")
        refused(fn(_args(offsets=(1, 3, 8))), "seq_offsets[0] = 1")
        refused(fn(_args(offsets=(0, 5, 4, 8))), "seq_offsets[2] = 4")
        refused(fn(_args(offsets=(0, 3, 7))), "seq_offsets[2] = 7", "n_windows 8")
        refused(fn(_args(offsets=(0, 3, 9))), "seq_offsets[2] = 9")
        rc = fn(_args(workspace_bytes=100))                                                   # a workspace too small has its own code
        assert rc == -4 and "100 B" in _capi.last_error() and name in _capi.last_error()
    emit = lib.avexhip_events_emit
    refused(emit(C.byref(_args()), None, None), "events_emit", "null")
    refused(emit(C.byref(_args()), C.byref(_result(capacity=-1)), None), "capacity -1")
    for field in ("sequence", "class_id", "first", "last", "peak", "peak_window", "mean"):
        refused(emit(C.byref(_args()), C.byref(_result(**{field: None})), None), "null output")
    refused(lib.avexhip_events_scan(None, None), "null")


# ------------------------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture()
def no_gpu(monkeypatch):
    """Whatever reaches the device fails the test: every ValueError below is raised before _capi.require_gpu()."""
    def boom():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_capi, "require_gpu", boom)


class _Windows:
    """What decode_events reads of a RecordingWindows."""
    n_windows = 6
    ranges = [(0, 2), (2, 6)]
    start_s = np.arange(6) * 0.5
    end_s = np.arange(6) * 0.5 + 1.0


def test_decode_events_errors(no_gpu):
    x = np.zeros((6, 3), dtype=np.float32)
    ok = dict(on=0.5)
    for bad in (np.zeros(6, dtype=np.float32), np.zeros((6, 3, 1), dtype=np.float32), np.zeros((6, 0), dtype=np.float32), np.zeros((6, 3), dtype=np.int64),
                torch.zeros(6, 3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            detection.decode_events(bad, **ok)
    for kw in (dict(smooth=0), dict(smooth=2), dict(smooth=33), dict(smooth=3.0), dict(smooth=True), dict(smooth_mode="max"), dict(smooth_mode=None),
               dict(merge_gap=-1), dict(merge_gap=65), dict(merge_gap=1.5), dict(min_windows=0), dict(min_windows=65), dict(min_windows=None),
               dict(max_events=-1), dict(max_events=2.5), dict(max_events=True), dict(activation="softmax"), dict(activation="Sigmoid")):
        with pytest.raises(ValueError):
            detection.decode_events(x, **ok, **kw)
        with pytest.raises(ValueError):
            detection.detect_events(None, lambda e: e, ["a.wav"], 1.0, **ok, **kw)
    for kw in (dict(on=None), dict(on=[0.5, 0.5]), dict(on=0.5, off=[0.1] * 4), dict(on=0.5, off=0.6), dict(on=[0.5, 0.5, 0.5], off=[0.1, 0.6, 0.1]),
               dict(on=float("nan")), dict(on=0.5, off=float("nan")), dict(on="high"), dict(on=np.zeros((3, 1))),
               dict(on=1.0, activation="sigmoid"), dict(on=0.5, off=0.0, activation="sigmoid"), dict(on=1.5, activation="sigmoid")):
        with pytest.raises(ValueError):
            detection.decode_events(x, **kw)
    with pytest.raises(ValueError, match="class 1"):
        detection.decode_events(x, on=[0.5, 0.5, 0.5], off=[0.1, 0.6, 0.1])
    for off in ([1, 6], [0, 4, 3, 6], [0, 5], [0, 7], [0], [[0, 6]], [0.0, 6.0]):
        with pytest.raises(ValueError):
            detection.decode_events(x, seq_offsets=off, **ok)
    with pytest.raises(ValueError, match="not both"):
        detection.decode_events(x, seq_offsets=[0, 6], windows=_Windows(), **ok)
    with pytest.raises(ValueError, match="6 windows"):
        detection.decode_events(np.zeros((5, 3), dtype=np.float32), windows=_Windows(), **ok)
    for rows in ([0, 1, 6], [0, -2, 1], [[0, 1]], [0.0, 1.0]):
        with pytest.raises(ValueError):
            detection.decode_events(x, row_of_window=rows, **ok)
    with pytest.raises(ValueError):
        detection.decode_events(x, row_of_window=[0, 1, -1, 2], seq_offsets=[0, 5], **ok)    # four windows, offsets that end at five


def test_detect_events_errors_signatures_and_exports(no_gpu):
    for kw in (dict(on=None), dict(on=0.5, off=0.6), dict(on=0.5, probe_batch_size=0), dict(on=0.5, probe_batch_size=2.5)):
        with pytest.raises(ValueError):
            detection.detect_events(None, lambda e: e, ["a.wav"], 1.0, **kw)
    with pytest.raises(ValueError):
        detection.detect_events(None, "not callable", ["a.wav"], 1.0, on=0.5)
    with pytest.raises(ValueError, match="no recordings"):
        detection.detect_events(None, lambda e: e, [], 1.0, on=0.5)
    with pytest.raises(ValueError):
        detection.detect_events(None, lambda e: e, ["a.wav"], 1.0, on=0.5, tail="keep")
    with pytest.raises(ValueError):
        detection.detect_events(None, lambda e: e, ["a.wav"], 0.0, on=0.5)
    sig = inspect.signature(detection.decode_events)
    assert list(sig.parameters) == ["scores", "seq_offsets", "windows", "on", "off", "activation", "smooth", "smooth_mode", "merge_gap", "min_windows",
                                    "row_of_window", "max_events"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in sig.parameters.items() if name != "scores")
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["smooth"], d["smooth_mode"], d["merge_gap"], d["min_windows"], d["off"], d["activation"], d["max_events"]) == (1, "median", 0, 1, None, None, None)
    sig = inspect.signature(detection.detect_events)
    assert list(sig.parameters)[:5] == ["model", "probe", "sources", "window_s", "hop_s"] and sig.parameters["hop_s"].default is None
    assert sig.parameters["probe_batch_size"].default == 4096 and sig.parameters["return_scores"].default is False
    assert sig.parameters["probe_batch_size"].kind is inspect.Parameter.KEYWORD_ONLY
    from avex_amd import recordings
    gate = inspect.signature(recordings.embed_recordings).parameters
    for name in ("layers", "aggregation", "batch_size", "min_rms_db", "min_peak_db", "tail", "batch_invariant", "sr", "res_type", "device"):
        assert sig.parameters[name].default == gate[name].default, name
    import avex_amd
    assert avex_amd.decode_events is detection.decode_events and avex_amd.detect_events is detection.detect_events
    assert "decode_events" in avex_amd.__all__ and "detect_events" in avex_amd.__all__
