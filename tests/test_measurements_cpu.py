"""Event measurements without a GPU: the ABI number and the bindings, MeasureSpec's validation, the frame plan against a brute-force
count, the argument checks that refuse before any launch, closed forms on the NumPy restatement (tests/_measure_ref.py), the Raven round
trip, and the input condition the GPU decision test relies on, asserted from float64 alone."""
import math

import numpy as np
import pytest

import _activity_ref as A
import _measure_ref as M
import _soundscape_ref as S
from avex_amd import _capi, measurements
from avex_amd.annotations import Annotations
from avex_amd.measurements import MeasureSpec

SR = A.SR


def test_abi_version_and_bindings(built_lib):
    assert _capi.header_abi_version() >= 24
    for name in ("avexhip_measure_partials_bytes", "avexhip_measure_frames", "avexhip_measure_reduce"):
        assert name in _capi.SYMBOLS and hasattr(built_lib, name)
    assert built_lib.avexhip_measure_partials_bytes(0) == 0 and built_lib.avexhip_measure_partials_bytes(-1) == 0
    assert built_lib.avexhip_measure_partials_bytes(1 << 31) == 0
    assert built_lib.avexhip_measure_partials_bytes(3) == 3 * (257 + 1) * 4
    assert measurements.EVENT_DTYPE.itemsize == 64 and measurements.RESULT_DTYPE.itemsize == 12 * 8
    assert measurements.INT_COLUMNS == M.INTS and set(measurements.FLOAT_COLUMNS) <= set(M.FLOATS)
    import avex_amd
    from avex_amd import detection
    import inspect
    for name in ("MeasureSpec", "measure_boxes", "measure_events", "noise_spectrum", "write_raven"):
        assert name in avex_amd.__all__ and getattr(avex_amd, name) is getattr(measurements, name)
    assert inspect.signature(detection.detect_events).parameters["measure"].default is None


def test_struct_layouts_match_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{root}/include/avexhip.h"', "int main(void){"]
    want = {}
    for cname, dt in (("avexhip_measure_event", measurements.EVENT_DTYPE), ("avexhip_measure_result", measurements.RESULT_DTYPE)):
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        want[cname] = dt.itemsize
        for fname in dt.names:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
            want[f"{cname}.{fname}"] = dt.fields[fname][1]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert {k: int(v) for k, v in out.items()} == want


def test_spec_defaults_and_refusals():
    s = MeasureSpec()
    assert (s.hop, s.band, s.energy_fraction) == (128, None, 0.9) and not s.per_class
    assert s.levels == ((1.0 - 0.9) / 2.0, 0.5, 1.0 - (1.0 - 0.9) / 2.0) == M.levels(0.9)
    assert s.bins(SR).tolist() == [[0, 257]]
    with pytest.raises(Exception):
        s.hop = 256                                                     # immutable
    for kw in (dict(hop=31), dict(hop=513), dict(hop=128.0), dict(hop=True), dict(energy_fraction=0.0), dict(energy_fraction=1.0), dict(energy_fraction=-0.5),
               dict(energy_fraction=math.nan), dict(energy_fraction="most"), dict(energy_fraction=True), dict(band=(2000, 2000)), dict(band=(-1, 5)),
               dict(band=2000), dict(band=(1, 2, 3)), dict(band="wide"), dict(band=()), dict(band=[(1000, 2000), (3000, 2000)]), dict(band=(1, math.nan)),
               dict(band=[(1000, 2000), None])):
        with pytest.raises(ValueError):
            MeasureSpec(**kw)
    one = MeasureSpec(hop=256, band=(2000, 8000), energy_fraction=0.5)
    assert one.band == (2000.0, 8000.0) and not one.per_class and one.bins(SR).tolist() == [[64, 256]] and one.levels == (0.25, 0.5, 0.75)
    per = MeasureSpec(band=[(2000, 8000), [1000.0, 4001.0]])
    assert per.per_class and per.band == ((2000.0, 8000.0), (1000.0, 4001.0)) and per.bins(SR).tolist() == [list(b) for b in A.bins(per.band, SR)] == [[64, 256], [32, 129]]
    assert MeasureSpec(band=[(0, 8001)]).per_class and MeasureSpec(band=[(0, 8001)]).bins(SR).tolist() == [[0, 257]]
    with pytest.raises(ValueError):
        MeasureSpec(band=(9000, 10000)).bins(SR)                        # past Nyquist
    with pytest.raises(ValueError):
        MeasureSpec(band=(2001, 2002)).bins(SR)                         # between two bins
    with pytest.raises(TypeError):
        measurements.measure_boxes(None, [0], [0], [512], "spec")


@pytest.mark.parametrize("hop", [32, 200, 256, 512])
def test_event_frames_against_a_brute_force_count(hop):
    n = 40001
    F = A.n_frames_of(n, hop)
    last = (F - 1) * hop
    boxes = [(0, 511), (100, 400), (1000, 1511),                       # shorter than 512 samples
             (0, 512), (1000, 1512), (hop * 3, hop * 3 + 512), (hop * 3 + 1, hop * 3 + 513), (n - 512, n),      # exactly 512 samples
             (0, 513), (0, 5000), (0, n),                               # starting at 0
             (30000, n), (n - 513, n), (last, n), (last - 1, n), (1, n),       # ending at the recording's last sample
             (last, last + 512), (last + 1, n), (n - 100, n), (n, n), (0, 0), (777, 777), (5000, 5000 + 64 * hop + 512 - hop), (123, 39999)]
    s0, s1 = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    f0, cnt = measurements.event_frames(s0, s1, hop, np.full(len(boxes), n))
    assert f0.dtype == np.int64 and cnt.dtype == np.int64
    for i, (a, b) in enumerate(boxes):
        assert (int(f0[i]), int(cnt[i])) == M.event_frames(a, b, hop, n), (hop, a, b)
    assert cnt[:3].tolist() == [0, 0, 0] and cnt[3] == 1 and cnt[10] == F
    # past F_r: the recording is shorter than the box claims to need (a box is cut at the recording's frames)
    f0, cnt = measurements.event_frames([0, 0, 300], [n, n, 512], hop, [n, 511, 600])
    assert cnt.tolist() == [F, 0, 0]
    f0, cnt = measurements.event_frames([0], [10 ** 6], hop, [n])       # a box that claims more samples than the recording has
    assert cnt.tolist() == [F]
    assert [int(v) for v in measurements.event_frames(7, 9000, hop, n)] == list(M.event_frames(7, 9000, hop, n))      # scalars


def _table(boxes, hop, n_samples=(40001, 511, 6000)):
    """boxes: (recording, s0, s1, lo, hi)."""
    base = np.cumsum([0] + [(v + 3) & ~3 for v in n_samples[:-1]])
    ev = np.zeros(len(boxes), dtype=measurements.EVENT_DTYPE)
    for e, (r, a, b, lo, hi) in enumerate(boxes):
        ev[e]["base"], ev[e]["n_samples"], ev[e]["s0"], ev[e]["s1"], ev[e]["lo"], ev[e]["hi"], ev[e]["recording"] = base[r], n_samples[r], a, b, lo, hi, r
    _, n = measurements.event_frames(ev["s0"], ev["s1"], hop, ev["n_samples"])
    runs = (n + 63) // 64
    ev["n_frames"], ev["env_offset"], ev["first_run"] = n, np.cumsum(n) - n, np.cumsum(runs) - runs
    return ev, int(n.sum()), int(runs.sum()), int(base[-1] + n_samples[-1])


def test_entry_points_refuse_before_any_launch(built_lib):
    """Every refusal comes from the host checks: the pointers below are made up, so no call here may pass them -- with a device present
    it would launch over them."""
    L = built_lib
    ev, F, runs, total = _table([(0, 0, 40001, 0, 257), (1, 0, 511, 0, 257), (2, 1000, 6000, 64, 256), (0, 200, 20000, 256, 257)], 200)
    assert ev["n_frames"].tolist() == [198, 0, 23, 97] and (F, runs) == (318, 4 + 0 + 1 + 2)
    host, dev, buf = ev.ctypes.data, 0x1000, 0x10000
    pb = L.avexhip_measure_partials_bytes(runs)
    assert pb == runs * 258 * 4

    def frames(**kw):
        a = dict(wav=buf, wav_samples=total, host=host, dev=dev, n=4, hop=200, tab=buf, F=F, runs=runs, part=buf, pb=pb, env=buf)
        a.update(kw)
        return L.avexhip_measure_frames(a["wav"], a["wav_samples"], a["host"], a["dev"], a["n"], a["hop"], a["tab"], a["F"], a["runs"], a["part"], a["pb"], a["env"], None)

    for kw in (dict(wav=None), dict(tab=None), dict(host=None), dict(dev=None), dict(part=None), dict(env=None), dict(wav=buf + 4), dict(tab=buf + 8),
               dict(dev=dev + 4), dict(part=buf + 2), dict(env=buf + 1), dict(hop=31), dict(hop=513), dict(n=-1), dict(wav_samples=total - 1),
               dict(wav_samples=0), dict(F=F + 1), dict(runs=runs - 1), dict(hop=256)):
        assert frames(**kw) == -1 and _capi.last_error().startswith("measure_frames:"), kw
    assert frames(pb=pb - 4) == -4 and "runs need" in _capi.last_error()

    res = np.zeros(1, dtype=measurements.RESULT_DTYPE)
    for name in res.dtype.names:
        res[name][0] = buf

    def reduce(**kw):
        a = dict(host=host, dev=dev, n=4, hop=200, F=F, runs=runs, part=buf, pb=pb, env=buf, noise=None, n_rec=3, q=(0.05, 0.5, 0.95), spec=buf, res=res)
        a.update(kw)
        return L.avexhip_measure_reduce(a["host"], a["dev"], a["n"], a["hop"], a["F"], a["runs"], a["part"], a["pb"], a["env"], a["noise"], a["n_rec"], *a["q"],
                                        a["spec"], a["res"].ctypes.data if a["res"] is not None else None, None)

    def without(column, value=0):
        r = res.copy()
        r[column][0] = value
        return r

    for kw in (dict(host=None), dict(dev=None), dict(dev=dev + 4), dict(part=None), dict(env=None), dict(spec=None), dict(res=None), dict(part=buf + 2),
               dict(env=buf + 1), dict(spec=buf + 2), dict(noise=buf + 2), dict(hop=16), dict(n=-2), dict(F=F - 1), dict(runs=runs + 1),
               dict(q=(0.0, 0.5, 0.95)), dict(q=(0.05, 0.5, 1.0)), dict(q=(0.6, 0.5, 0.95)), dict(q=(0.05, 0.97, 0.95)), dict(q=(math.nan, 0.5, 0.95)),
               dict(q=(0.05, 0.5, math.nan)), dict(noise=buf, n_rec=0), dict(noise=buf, n_rec=2),       # an event of recording 2
               dict(res=without("energy")), dict(res=without("peak_frame")), dict(res=without("snr_db", buf + 4)), dict(res=without("low_bin", buf + 2))):
        assert reduce(**kw) == -1 and _capi.last_error().startswith("measure_reduce:"), kw
    assert reduce(pb=pb - 1) == -4

    def changed(e, field, value):
        bad = ev.copy()
        bad[field][e] = value
        return bad

    for bad in (changed(2, "n_frames", 22), changed(2, "first_run", 5), changed(3, "env_offset", 220), changed(1, "n_samples", 0), changed(1, "base", -4),
                changed(0, "s1", 40002), changed(0, "s0", -1), changed(2, "s1", 999), changed(2, "lo", -1), changed(2, "hi", 258), changed(2, "hi", 64),
                changed(3, "lo", 257), changed(0, "recording", -1), changed(2, "base", total)):
        assert frames(host=bad.ctypes.data) == -1, _capi.last_error()
        if int(bad["base"][2]) != total:                                # (reduce has no buffer to check a base against and would launch)
            assert reduce(host=bad.ctypes.data) == -1
    # an event of more than 2^24 frames
    big, Fb, rb, tb = _table([(0, 0, 32 * ((1 << 24) + 1) + 480, 0, 257)], 32, n_samples=(32 * ((1 << 24) + 1) + 480,))
    assert int(big["n_frames"][0]) == (1 << 24) + 1
    rc = L.avexhip_measure_frames(buf, tb, big.ctypes.data, dev, 1, 32, buf, Fb, rb, buf, L.avexhip_measure_partials_bytes(rb), buf, None)
    assert rc == -1 and "more than 16777216" in _capi.last_error()
    # no event at all, and no event that holds a frame: success, and nothing to launch
    assert L.avexhip_measure_frames(None, 0, None, None, 0, 200, None, 0, 0, None, 0, None, None) == 0
    assert L.avexhip_measure_reduce(None, None, 0, 200, 0, 0, None, 0, None, None, 0, 0.05, 0.5, 0.95, None, None, None) == 0
    none, F0, r0, t0 = _table([(1, 0, 511, 0, 257), (0, 100, 400, 3, 4)], 256)
    assert (F0, r0) == (0, 0)
    assert L.avexhip_measure_frames(buf, t0, none.ctypes.data, dev, 2, 256, buf, 0, 0, None, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------------------- closed forms
def test_a_full_scale_sine_on_bin_96():
    """Under the periodic Hann window a bin-centred sine puts |X|^2 = 128^2 on its bin and a quarter of that on each neighbour: the
    cumulative shares are 1/6, 5/6, 1, so at p = 0.9 the bounds are bins 95 and 97, the centre and the peak bin 96."""
    hop, n = 256, 512 + 256 * 9
    x = np.sin(2.0 * np.pi * 96 * np.arange(n) / 512.0).astype(np.float32)
    r = M.measure_box(A.frame_power64(x, hop), 0, n, 0, 257, hop, SR, n)
    assert (r["n_frames"], r["nonfinite"], r["first_frame"]) == (10, 0, 0)
    assert (r["low_bin"], r["centre_bin"], r["high_bin"], r["peak_bin"]) == (95, 96, 97, 96)
    assert abs(r["spectrum"][96] / 10 - 128.0 ** 2) < 1e-2 and abs(r["spectrum"][95] / r["spectrum"][96] - 0.25) < 1e-6
    assert (r["low_hz"], r["centre_hz"], r["high_hz"], r["peak_hz"], r["bandwidth_hz"]) == (95 * 31.25, 3000.0, 97 * 31.25, 3000.0, 3 * 31.25)
    # a steady tone: the time bounds hold the middle 90 % of ten equal frames; the centre is a tie between frames 4 and 5 that rounding decides
    assert (r["low_frame"], r["high_frame"]) == (0, 9) and r["centre_frame"] in (4, 5) and r["begin_s"] == 0.0 and r["end_s"] == (9 * 256 + 512) / SR
    assert r["duration_s"] == r["end_s"] - r["begin_s"] and r["centre_s"] == (r["centre_frame"] * 256 + 256) / SR and math.isnan(r["snr_db"])
    inside = M.measure_box(A.frame_power64(x, hop), 0, n, 96, 97, hop, SR, n)       # a one-bin band
    assert (inside["low_bin"], inside["centre_bin"], inside["high_bin"], inside["peak_bin"]) == (96, 96, 96, 96) and inside["bandwidth_hz"] == 31.25
    assert (inside["spectrum"][:96] == 0).all() and (inside["spectrum"][97:] == 0).all()


def test_a_single_click_gives_its_frames():
    """hop 128: a click at sample 5000 lies in frames 36..39 (36 * 128 = 4608 <= 5000 < 39 * 128 + 512); where the window is largest,
    frame 37 (the click at 264 of 512), the envelope peaks.  The squared window at 392, 264, 136 and 8 is 0.203, 0.995, 0.301 and 6e-6:
    cumulative shares 0.135, 0.799, 1.000, 1.000, so the 5 %, 50 % and 95 % frames are 36, 37 and 38."""
    hop, n = 128, 16000
    x = np.zeros(n, np.float32)
    x[5000] = 1.0
    r = M.measure_box(A.frame_power64(x, hop), 2000, 12000, 0, 257, hop, SR, n)
    assert r["first_frame"] == 16 and r["n_frames"] == (12000 - 512) // 128 + 1 - 16
    e = r["envelope"]
    assert np.flatnonzero(e > 1e-9).tolist() == [36 - 16, 37 - 16, 38 - 16, 39 - 16]
    assert r["peak_frame"] == 37 and (r["low_frame"], r["centre_frame"], r["high_frame"]) == (36, 37, 38)
    assert r["begin_s"] == 36 * 128 / SR and r["end_s"] == (38 * 128 + 512) / SR and r["begin_s"] <= 5000 / SR < r["end_s"]
    assert r["peak_s"] == (37 * 128 + 256) / SR


def test_silence_a_short_box_and_a_nan():
    hop, n = 256, 4096
    P = A.frame_power64(np.zeros(n, np.float32), hop)
    r = M.measure_box(P, 0, n, 0, 257, hop, SR, n)
    assert r["n_frames"] == 15 and r["energy"] == 0.0 and (r["spectrum"] == 0).all() and (r["envelope"] == 0).all()
    for k in M.INTS[2:]:
        assert r[k] == -1, k
    for k in M.FLOATS[1:]:
        assert math.isnan(r[k]), k
    short = M.measure_box(P, 100, 600, 0, 257, hop, SR, n)             # 500 samples: no frame
    assert short["n_frames"] == 0 and math.isnan(short["energy"]) and all(short[k] == -1 for k in M.INTS[2:])
    x = A.synthetic()[:n].copy()
    x[2000] = np.nan
    bad = M.measure_box(A.frame_power64(x, hop), 0, n, 32, 129, hop, SR, n)
    assert bad["nonfinite"] == 2 and np.isnan(bad["spectrum"][32:129]).all() and (bad["spectrum"][:32] == 0).all() and math.isnan(bad["energy"])
    assert all(bad[k] == -1 for k in M.INTS[2:]) and np.isnan(bad["envelope"]).sum() == 2
    clean = M.measure_box(A.frame_power64(x, hop), 2048, n, 32, 129, hop, SR, n)
    assert clean["nonfinite"] == 0 and clean["low_bin"] >= 32 and clean["high_bin"] < 129 and clean["first_frame"] == 8


def test_noise_subtraction():
    """noise = spectrum / n takes everything off: with n = 64 the division and the product are exact, so the energy is exactly 0 (for
    another n, fl32(spectrum / n) n may lie one rounding below spectrum).  Half of it leaves half, and 3.01 dB."""
    hop, n = 256, 512 + 256 * 63
    x = A.synthetic()[10000:10000 + n]
    P = A.frame_power64(x, hop)
    plain = M.measure_box(P, 0, n, 0, 257, hop, SR, n)
    assert plain["n_frames"] == 64
    spectrum = plain["spectrum"].astype(np.float32)
    noise = (spectrum / np.float32(64)).astype(np.float32)
    r = M.measure(spectrum, plain["envelope"].astype(np.float32), 0, 0, 0, 257, hop, SR, noise=noise)
    assert r["energy"] == 0.0 and r["snr_db"] == -math.inf and all(r[k] == -1 for k in ("low_bin", "centre_bin", "high_bin", "peak_bin"))
    assert math.isnan(r["low_hz"]) and math.isnan(r["bandwidth_hz"])
    half = M.measure(spectrum, plain["envelope"].astype(np.float32), 0, 0, 0, 257, hop, SR, noise=noise / np.float32(2))
    assert abs(half["energy"] / float(spectrum.astype(np.float64).sum()) - 0.5) < 1e-12 and abs(half["snr_db"] - 10 * math.log10(1.0)) < 1e-9
    assert half["peak_bin"] == plain["peak_bin"]
    zero = M.measure(spectrum, plain["envelope"].astype(np.float32), 0, 0, 0, 257, hop, SR, noise=np.zeros(257, np.float32))
    assert math.isnan(zero["snr_db"]) and zero["energy"] == float(np.cumsum(spectrum.astype(np.float64))[-1])
    ns = M.noise_spectrum(np.array([[3.0] * 257, [1.0] * 257, [0.5] * 257, [2.0] * 257], np.float32), [4, 4, 2, 4], [0, 0, 0, 1], [0, 0, 0, 1], 4, 3)
    assert (ns[0] == 1.0).all() and np.isnan(ns[1]).all() and np.isnan(ns[2]).all()


# ------------------------------------------------------------------------------------------------------------- Raven tables
def test_write_raven_reads_back(tmp_path):
    t = [0.1 + 0.2, 1.0 / 3.0, 2.5, 12.345678901234567]
    events = {"sequence": np.array([0, 0, 1, 0, -1], np.int32), "class_id": np.array([1, 0, 1, 1, -1], np.int32), "first": np.array([0, 2, 5, 7, -1], np.int32),
              "last": np.array([1, 3, 6, 8, -1], np.int32), "peak": np.array([0.9, 0.5, 0.7, 0.25, -np.inf], np.float32),
              "start_s": np.array([0.0, 5.0, 2.5, 17.5, np.nan]), "end_s": np.array([7.5, 12.5, 10.0, 25.0, np.nan])}
    m = {"low_frame": np.array([3, -1, 4, 9, -1], np.int32), "high_frame": np.array([8, -1, 6, 30, -1], np.int32), "low_bin": np.array([95, -1, 10, -1, -1], np.int32),
         "high_bin": np.array([97, -1, 20, -1, -1], np.int32), "begin_s": np.array([t[0], np.nan, 1.0, t[1], np.nan]), "end_s": np.array([t[3], np.nan, 2.0, t[2], np.nan]),
         "low_hz": np.array([95 * 31.25, np.nan, 312.5, np.nan, np.nan]), "high_hz": np.array([97 * 31.25, np.nan, 625.0, np.nan, np.nan])}
    path = tmp_path / "rec0.txt"
    assert measurements.write_raven(path, events, m, recording=0, class_names=["chiff", "chaff"], sr=SR) == 3
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["Selection", "View", "Channel", "Begin Time (s)", "End Time (s)", "Low Freq (Hz)", "High Freq (Hz)", "Species", "Score"]
    rows = [l.split("\t") for l in lines[1:]]
    assert [r[0] for r in rows] == ["1", "2", "3"] and [r[7] for r in rows] == ["chaff", "chiff", "chaff"]
    assert [float(r[5]) for r in rows] == [95 * 31.25, 0.0, 0.0] and [float(r[6]) for r in rows] == [97 * 31.25, 8000.0, 8000.0]
    assert [float(r[8]) for r in rows] == [float(np.float32(v)) for v in (0.9, 0.5, 0.25)]
    back = Annotations.from_raven([path], class_column="Species", class_names=["chiff", "chaff"])
    assert back.recording.tolist() == [0, 0, 0] and back.class_id.tolist() == [1, 0, 1]
    assert back.start_s.tolist() == [t[0], 5.0, t[1]] and back.end_s.tolist() == [t[3], 12.5, t[2]]      # exact: repr round-trips a float64
    other = tmp_path / "rec1.txt"
    assert measurements.write_raven(other, events, m, recording=1, class_column="Call") == 1
    both = Annotations.from_raven([other], class_column="Call", recording=[1])
    assert both.recording.tolist() == [1] and both.start_s.tolist() == [1.0] and both.end_s.tolist() == [2.0] and both.class_names == ("1",)
    plain = tmp_path / "plain.txt"                                      # without measurements: the window spans
    assert measurements.write_raven(plain, events, recording=0) == 3
    back = Annotations.from_raven([plain], class_column="Species")
    assert back.start_s.tolist() == [0.0, 5.0, 17.5] and back.end_s.tolist() == [7.5, 12.5, 25.0]
    assert measurements.write_raven(tmp_path / "none.txt", events, m, recording=7) == 0
    assert len(Annotations.from_raven([tmp_path / "none.txt"], class_column="Species")) == 0
    with pytest.raises(ValueError):
        measurements.write_raven(plain, events, {k: v[:3] for k, v in m.items()}, recording=0)


# ------------------------------------------------------------------------------------------------------------- the decision test's inputs
@pytest.mark.parametrize("hop", A.HOPS)
def test_decisions_have_a_margin(hop):
    """What tests/test_gpu_measurements.py's decision test relies on, from the float64 reference and the float32 CPU chain alone: on the
    synthetic recording, for the boxes and bands of _measure_ref, every bin and frame quantile at p = 0.9 stands at least 1e-4 of the
    total away from its level (at the chosen index and the one before), and the float32 CPU chain chooses the same indices."""
    x = A.synthetic()
    P64, P32 = A.frame_power64(x, hop), S.power32(x, hop)
    worst = math.inf
    for s0, s1 in M.BOXES:
        for lo, hi in M.BANDS:
            r64 = M.measure_box(P64, s0, s1, lo, hi, hop, SR, len(x))
            r32 = M.measure_box(P32, s0, s1, lo, hi, hop, SR, len(x))
            assert r64["n_frames"] >= 2 and len(r64["margins"]) == 6
            worst = min(worst, min(r64["margins"]))
            for k in ("low_bin", "centre_bin", "high_bin", "peak_bin", "low_frame", "centre_frame", "high_frame"):
                assert r64[k] == r32[k] and r64[k] >= 0, (s0, s1, lo, hi, k)
    print(f"hop {hop}: the smallest margin is {worst:.3e}")
    assert worst >= 1e-4
