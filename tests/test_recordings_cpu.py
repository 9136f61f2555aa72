"""avex_amd.recordings without a GPU: the window plan, the row / mask semantics of the restatement the GPU tests compare against, and
the ABI 14 bindings."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _recordings_ref as R
from avex_amd import _capi, recordings


def test_plan_hand_written_cases():
    P = recordings.plan_recording_windows

    def plan(*a, **k):
        s, v = P(*a, **k)
        assert s.dtype == v.dtype == np.int64
        return s.tolist(), v.tolist()

    assert plan(100, 100, 30, "pad") == ([0, 30, 60, 90], [100, 70, 40, 10])
    assert plan(100, 100, 30, "drop") == ([0], [100])
    for tail in ("pad", "drop"):
        assert plan(7, 100, 30, tail) == ([0], [7])                      # n < window: one padded window under both
    assert plan(100, 100, 100) == ([0], [100])                           # n = window, no overlap: one full window
    assert plan(101, 100, 100, "pad") == ([0, 100], [100, 1])            # n = window + 1: a second window with valid = 1 ...
    assert plan(101, 100, 100, "drop") == ([0], [100])                   # ... absent under drop
    assert plan(10, 3, 7, "pad") == ([0, 7], [3, 3])                     # hop > window: samples 3..6 are in no window
    assert plan(11, 3, 7, "pad") == ([0, 7], [3, 3]) and plan(15, 3, 7, "pad") == ([0, 7, 14], [3, 3, 1])
    assert plan(15, 3, 7, "drop") == ([0, 7], [3, 3])
    assert plan(5, 3, 1, "pad") == ([0, 1, 2, 3, 4], [3, 3, 3, 2, 1])    # hop = 1
    assert plan(5, 3, 1, "drop") == ([0, 1, 2], [3, 3, 3])
    assert plan(1, 1, 1) == ([0], [1])


@pytest.mark.parametrize("tail", ["pad", "drop"])
def test_plan_matches_the_restatement(tail):
    for n in (1, 2, 63, 64, 65, 1000, 4001, 4002, 18141):
        for w in (1, 64, 1000, 4001):
            for h in (1, 16, 63, 907, 1237, 5000):
                if n // h > 5000:
                    continue
                s, v = recordings.plan_recording_windows(n, w, h, tail)
                rs, rv = R.plan(n, w, h, tail)
                assert s.tolist() == rs and v.tolist() == rv, (n, w, h, tail)
                assert len(s) >= 1 and (v >= 1).all() and (s + v <= n).all() and (s < n).all()


def test_plan_errors():
    P = recordings.plan_recording_windows
    for bad in ((0, 10, 5), (-3, 10, 5), (10, 0, 5), (10, -1, 5), (10, 10, 0), (10, 10, -2)):
        with pytest.raises(ValueError):
            P(*bad)
        with pytest.raises(ValueError):
            R.plan(*bad)
    for tail in ("keep", "", None, "PAD"):
        with pytest.raises(ValueError):
            P(10, 4, 2, tail)
    with pytest.raises(ValueError):
        recordings._to_len(0.0, 16000, "window_s")


def test_restated_rows_are_slice_then_pad():
    """The reference's pad_or_window(wav[start:], window_len, "start"), written out: the slice, F.pad with zeros behind it, mask True on
    the padding."""
    x = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    for w, h, tail in ((64, 16, "pad"), (300, 301, "pad"), (999, 1, "drop"), (1000, 7, "pad"), (1500, 100, "drop")):
        starts, valids = R.plan(len(x), w, h, tail)
        wav, mask = R.rows(x, starts, valids, w)
        t = torch.from_numpy(x)
        for b, s in enumerate(starts):
            seg = t[s:][:w]
            assert torch.equal(torch.from_numpy(wav[b]), F.pad(seg, (0, w - seg.numel())))
            assert torch.equal(torch.from_numpy(mask[b]), torch.arange(w) >= seg.numel())
            assert seg.numel() == valids[b]


def test_restated_statistics_and_gate():
    x = np.zeros(40, dtype=np.float32)
    x[10:20] = 0.5
    x[30] = np.nan
    starts, valids = R.plan(40, 10, 10)
    e, p = R.stats(x, starts, valids)
    assert e[:3].tolist() == [0.0, 2.5, 0.0] and np.isnan(e[3]) and p[:3].tolist() == [0.0, 0.5, 0.0] and np.isnan(p[3])
    rms, pk = R.db(e, p, valids)
    assert rms[0] == -np.inf and abs(rms[1] - 20 * np.log10(0.5)) < 1e-12 and abs(pk[1] - 20 * np.log10(0.5)) < 1e-6
    assert R.select(e, p, valids) == [0, 1, 2]                          # no gate keeps everything but the NaN window
    assert R.select(e, p, valids, *R.thresholds(-12.0, None)) == [1] and R.select(e, p, valids, *R.thresholds(None, -3.0)) == []


def test_bindings(built_lib):
    assert _capi.header_abi_version() >= 14
    for name in ("avexhip_window_stats", "avexhip_window_select", "avexhip_window_gather"):
        assert name in _capi.SYMBOLS and hasattr(built_lib, name)
    assert C.sizeof(_capi.Window) == recordings.WINDOW_DTYPE.itemsize == 32
    for (name, _), off in zip(_capi.Window._fields_, (0, 8, 16, 24, 28)):
        assert getattr(_capi.Window, name).offset == recordings.WINDOW_DTYPE.fields[name][1] == off


def test_argument_checks_need_no_gpu(built_lib):
    """The entry points refuse a bad table before they touch the device, and name the window."""
    tab = np.zeros(3, dtype=recordings.WINDOW_DTYPE)
    tab["n_samples"], tab["start"], tab["valid"] = 100, (0, 40, 80), (40, 40, 21)
    fake = 1 << 20                                                       # a 16-byte aligned number: never dereferenced, the table is refused first
    rc = built_lib.avexhip_window_stats(fake, 100, tab.ctypes.data, fake, 3, 40, fake, fake, None)
    assert rc == -1 and "window 2" in _capi.last_error() and "leaves the recording" in _capi.last_error()
    rc = built_lib.avexhip_window_gather(fake, 100, tab.ctypes.data, fake, 3, None, 0, 4, 40, fake, 0, fake, None)
    assert rc == -1 and "leave the table" in _capi.last_error()
    rc = built_lib.avexhip_window_select(fake, fake, fake, 3, float("nan"), 0.0, fake, fake, None)
    assert rc == -1 and "NaN" in _capi.last_error()
