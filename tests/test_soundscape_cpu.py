"""Acoustic indices without a GPU: the ABI number, IndexSpec's validation, the segment plan against hand-worked cases, the bindings, the
argument checks that refuse before any launch, closed forms on the NumPy restatement (tests/_soundscape_ref.py), and the two input
conditions the GPU count test relies on, asserted from the float64 reference alone."""
import ctypes as C
import math

import numpy as np
import pytest

import _activity_ref as A
import _soundscape_ref as S
from avex_amd import _capi, soundscape
from avex_amd.soundscape import IndexSpec

SR = A.SR


def test_abi_version_and_bindings(built_lib):
    assert _capi.header_abi_version() >= 23
    for name in ("avexhip_soundscape_partials_bytes", "avexhip_soundscape_frames", "avexhip_soundscape_reduce", "avexhip_soundscape_indices"):
        assert name in _capi.SYMBOLS and hasattr(built_lib, name)
    assert built_lib.avexhip_soundscape_partials_bytes(0) == 0 and built_lib.avexhip_soundscape_partials_bytes(-1) == 0
    assert built_lib.avexhip_soundscape_partials_bytes(3) == 3 * (6 * 257 + 2) * 4
    assert soundscape.RECORDING_DTYPE.itemsize == 32 and soundscape.INDEX_SPEC_DTYPE.itemsize == 8 * 4 + 32 * 2 * 4 + 8
    assert soundscape.INDEX_NAMES == S.NAMES
    import avex_amd
    for name in ("IndexSpec", "acoustic_indices", "spectral_stats"):
        assert name in avex_amd.__all__ and getattr(avex_amd, name) is getattr(soundscape, name)


def test_struct_layouts_match_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{root}/include/avexhip.h"', "int main(void){"]
    want = {}
    for cname, dt in (("avexhip_soundscape_recording", soundscape.RECORDING_DTYPE), ("avexhip_soundscape_index_spec", soundscape.INDEX_SPEC_DTYPE)):
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
    s = IndexSpec()
    assert (s.hop, s.segment_s, s.db_threshold, s.band, s.bio_band, s.anthro_band, s.adi_step_hz, s.adi_max_hz) == \
        (256, 60.0, -50.0, None, (2000.0, 8000.0), (1000.0, 2000.0), 1000.0, 10000.0)
    assert s.segment_frames(16000) == 3750 and s.threshold == np.float32(16384.0 * 1e-5) == S.threshold(-50.0)
    assert IndexSpec(db_threshold=-math.inf).threshold == 0.0 and IndexSpec(db_threshold=math.inf).threshold == np.inf
    assert IndexSpec(db_threshold=5000).threshold == np.inf
    with pytest.raises(Exception):
        s.hop = 128                                                     # immutable
    for kw in (dict(hop=31), dict(hop=513), dict(hop=256.0), dict(hop=True), dict(segment_s=0), dict(segment_s=-1.0), dict(segment_s=math.inf),
               dict(db_threshold=math.nan), dict(db_threshold="loud"), dict(band=(2000, 2000)), dict(band=(-1, 5)), dict(band=2000), dict(band=(1, 2, 3)),
               dict(bio_band=(8000, 2000)), dict(bio_band=None), dict(anthro_band=(1, math.nan)), dict(adi_step_hz=0), dict(adi_max_hz=-5.0)):
        with pytest.raises(ValueError):
            IndexSpec(**kw)
    with pytest.raises(ValueError):
        IndexSpec(segment_s=0.001).segment_frames(16000)                # round(0.0625) = 0 frames
    assert IndexSpec(segment_s=0.009, hop=256).segment_frames(16000) == 1
    with pytest.raises(ValueError):
        IndexSpec(bio_band=(9000, 10000)).bins(16000)                   # past Nyquist
    with pytest.raises(ValueError):
        IndexSpec(band=(2001, 2002)).bins(16000)                        # between two bins
    with pytest.raises(ValueError):
        IndexSpec(adi_step_hz=100.0).bins(16000)                        # 80 bands
    with pytest.raises(ValueError):
        IndexSpec(adi_step_hz=9000.0).bins(16000)                       # none
    with pytest.raises(ValueError):
        IndexSpec(adi_step_hz=10.0, adi_max_hz=100.0).bins(16000)       # ten bands, but (10, 20) Hz holds no bin
    with pytest.raises(TypeError):
        soundscape.acoustic_indices(None, "spec")


def test_spec_bins():
    b = IndexSpec().bins(16000)
    assert b.dtype == soundscape.INDEX_SPEC_DTYPE and b.shape == (1,)
    assert b["band"][0].tolist() == [0, 257] and b["bio"][0].tolist() == [64, 256] and b["anthro"][0].tolist() == [32, 64]
    assert int(b["n_adi"][0]) == 8 and b["adi"][0, :8].tolist() == [[32 * j, 32 * j + 32] for j in range(8)]       # clipped to Nyquist: 8, not 10
    assert (b["adi"][0, 8:] == 0).all() and float(b["bin_khz"][0]) == 0.03125
    assert [list(x) for x in A.bins(S.adi_bands(S.Spec(), 16000), 16000)] == b["adi"][0, :8].tolist()
    b = IndexSpec(band=(500, 7000), adi_step_hz=8000, adi_max_hz=8000).bins(16000)
    assert b["band"][0].tolist() == [16, 224] and int(b["n_adi"][0]) == 1 and b["adi"][0, 0].tolist() == [0, 256]
    b = IndexSpec(adi_step_hz=2000, adi_max_hz=6500).bins(44100)
    assert int(b["n_adi"][0]) == 3 and b["adi"][0, :3].tolist() == [list(x) for x in A.bins([(0, 2000), (2000, 4000), (4000, 6000)], 44100)]


def test_segment_plan():
    hop, Sf = 200, 5
    n = [511, 512, 512 + 200 * 5, 512 + 200 * 4, 40001]                 # F = 0, 1, S + 1, S, 198
    plan = soundscape.segment_plan(n, hop, Sf, SR)
    assert plan["frames"].tolist() == [0, 1, 6, 5, 198] == [A.n_frames_of(v, hop) for v in n]
    assert plan["segments"].tolist() == [0, 1, 2, 1, 40]
    assert plan["segment_ranges"] == [(0, 0), (0, 1), (1, 3), (3, 4), (4, 44)] and plan["frame_ranges"] == [(0, 0), (0, 1), (1, 7), (7, 12), (12, 210)]
    assert plan["recording"].tolist() == [1, 2, 2, 3] + [4] * 40
    assert plan["n_frames"].tolist() == [1, 5, 1, 5] + [5] * 39 + [3]
    assert plan["first_frame"][:4].tolist() == [0, 0, 5, 0]
    # spans: the first frame's first sample .. the last frame's last sample
    assert plan["start_s"][:4].tolist() == [0.0, 0.0, 1000 / SR, 0.0] and plan["end_s"][:4].tolist() == [512 / SR, 1312 / SR, 1512 / SR, 1312 / SR]
    assert plan["end_s"][-1] == (197 * 200 + 512) / SR and plan["start_s"][-1] == 195 * 200 / SR
    for r, v in enumerate(n):
        g0, g1 = plan["segment_ranges"][r]
        want = S.spans_s(v, hop, Sf, SR)
        assert list(zip(plan["start_s"][g0:g1], plan["end_s"][g0:g1])) == want and plan["n_frames"][g0:g1].tolist() == [m for _, m in S.segments_of(A.n_frames_of(v, hop), Sf)]
    one = soundscape.segment_plan([6 * SR + 123], 256, 1000, SR)         # one S larger than F
    assert one["segments"].tolist() == [1] and one["n_frames"].tolist() == [374]
    with pytest.raises(ValueError):
        soundscape.segment_plan([1000], 256, 0, SR)


def _table(n_samples, hop, Sf):
    plan = soundscape.segment_plan(n_samples, hop, Sf, SR)
    rec = np.zeros(len(n_samples), dtype=soundscape.RECORDING_DTYPE)
    rec["n_samples"] = n_samples
    rec["base"] = np.cumsum([0] + [(v + 3) & ~3 for v in n_samples[:-1]])
    f, g = plan["frames"], plan["segments"]
    runs = (f // Sf) * ((Sf + 63) // 64) + (f % Sf + 63) // 64
    rec["first_frame"], rec["first_segment"], rec["first_run"] = np.cumsum(f) - f, np.cumsum(g) - g, np.cumsum(runs) - runs
    return rec, int(f.sum()), int(g.sum()), int(runs.sum())


def test_entry_points_refuse_before_any_launch(built_lib):
    """Every refusal comes from the host checks: the pointers below are never read on the device (this test runs without one)."""
    L = built_lib
    rec, F, G, runs = _table([40001, 511, 6000], 200, 150)
    assert (F, G, runs) == (198 + 28, 3, 3 + 1 + 1)
    host, dev, buf = rec.ctypes.data, 0x1000, 0x10000
    total = int(rec["base"][-1] + rec["n_samples"][-1])
    pb = L.avexhip_soundscape_partials_bytes(runs)

    def frames(**kw):
        a = dict(wav=buf, wav_samples=total, host=host, dev=dev, n_rec=3, hop=200, S=150, thr=1.0, tab=buf, F=F, G=G, part=buf, pb=pb, fp=buf)
        a.update(kw)
        return L.avexhip_soundscape_frames(a["wav"], a["wav_samples"], a["host"], a["dev"], a["n_rec"], a["hop"], a["S"], a["thr"], a["tab"], a["F"], a["G"],
                                           a["part"], a["pb"], a["fp"], None)

    cases = [dict(wav=None), dict(tab=None), dict(host=None), dict(dev=None), dict(part=None), dict(fp=None), dict(wav=buf + 4), dict(tab=buf + 8),
             dict(dev=dev + 4), dict(part=buf + 2), dict(fp=buf + 1), dict(hop=31), dict(hop=513), dict(S=0), dict(S=(1 << 24) + 1), dict(n_rec=0),
             dict(wav_samples=total - 1), dict(wav_samples=0), dict(F=F + 1), dict(G=G - 1), dict(thr=math.nan), dict(thr=-1.0), dict(hop=256), dict(S=64)]
    for kw in cases:
        assert frames(**kw) == -1 and _capi.last_error().startswith("soundscape_frames:"), kw
    assert frames(pb=pb - 4) == -4 and "runs need" in _capi.last_error()
    for field, value in (("first_frame", 1), ("first_segment", 1), ("first_run", 2), ("n_samples", 0), ("base", -4)):
        bad = rec.copy()
        bad[field][1] = value
        assert frames(host=bad.ctypes.data) == -1, field

    spec = IndexSpec().bins(SR)

    def indices(sp, **kw):
        a = dict(host=host, dev=dev, hop=200, S=150, F=F, G=G, out=buf)
        a.update(kw)
        return L.avexhip_soundscape_indices(a["host"], a["dev"], 3, a["hop"], a["S"], a["F"], a["G"], sp.ctypes.data if sp is not None else None, buf, buf, buf, buf, buf,
                                            buf, a["out"], None)

    def changed(field, value, at=None):
        sp = spec.copy()
        if at is None:
            sp[field][0] = value
        else:
            sp[field][0, at] = value
        return sp

    for sp in (None, changed("band", (0, 258)), changed("band", (5, 5)), changed("bio", (-1, 4)), changed("anthro", (70, 64)), changed("n_adi", 0),
               changed("n_adi", 33), changed("adi", (250, 258), at=7), changed("adi", (3, 3), at=0), changed("bin_khz", 0.0), changed("bin_khz", math.nan)):
        assert indices(sp) == -1 and _capi.last_error().startswith("soundscape_indices:")
    for kw in (dict(out=None), dict(out=buf + 4), dict(hop=16), dict(S=0), dict(G=G + 1), dict(dev=None)):
        assert indices(spec, **kw) == -1, kw
    assert L.avexhip_soundscape_reduce(host, dev, 3, 200, 150, F, G, buf, pb, buf, buf, None, buf, buf, None) == -1
    assert L.avexhip_soundscape_reduce(host, dev, 3, 200, 150, F, G, buf, pb - 1, buf, buf, buf, buf, buf, None) == -4
    assert L.avexhip_soundscape_reduce(host, dev, 3, 200, 150, F, G, buf, pb, buf, buf + 2, buf, buf, buf, None) == -1
    # no segment at all: success, and nothing to launch
    none, F0, G0, r0 = _table([511, 100], 256, 10)
    assert (F0, G0, r0) == (0, 0, 0)
    assert L.avexhip_soundscape_frames(buf, 700, none.ctypes.data, dev, 2, 256, 10, 1.0, buf, 0, 0, None, 0, None, None) == 0
    assert L.avexhip_soundscape_reduce(none.ctypes.data, dev, 2, 256, 10, 0, 0, None, 0, None, None, None, None, None, None) == 0
    assert L.avexhip_soundscape_indices(none.ctypes.data, dev, 2, 256, 10, 0, 0, spec.ctypes.data, None, None, None, None, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------------------- closed forms
def _seg(mean_power=None, mean_amplitude=None, abs_diff=None, count_above=None):
    z = np.zeros(257)
    return {"mean_power": z if mean_power is None else mean_power, "mean_amplitude": z if mean_amplitude is None else mean_amplitude,
            "abs_diff": z if abs_diff is None else abs_diff, "count_above": z.astype(np.int32) if count_above is None else count_above}


def _named(v):
    return dict(zip(S.NAMES, v))


def test_closed_forms_of_the_indices():
    spec, n = S.Spec(), 10
    J = len(S.adi_bands(spec, SR))
    assert J == 8
    # equal occupancy in every ADI band
    c = np.zeros(257, np.int32)
    c[:256] = 4
    r = _named(S.indices(_seg(count_above=c), np.ones(n), n, spec, SR))
    assert abs(r["adi"] - math.log(J)) < 1e-12 and abs(r["aei"]) < 1e-12
    # one occupied band of J
    c = np.zeros(257, np.int32)
    c[96:128] = 7
    r = _named(S.indices(_seg(count_above=c), np.ones(n), n, spec, SR))
    assert abs(r["aei"] - (J - 1) / J) < 1e-12 and r["adi"] == 0.0
    # power only in bio_band
    p = np.zeros(257)
    p[64:256] = 3.0
    r = _named(S.indices(_seg(mean_power=p), np.ones(n), n, spec, SR))
    assert r["ndsi"] == 1.0
    p = np.zeros(257)
    p[32:64] = 3.0
    assert _named(S.indices(_seg(mean_power=p), np.ones(n), n, spec, SR))["ndsi"] == -1.0
    # a flat spectrum, equal frame powers
    r = _named(S.indices(_seg(mean_power=np.full(257, 0.25)), np.full(n, 7.0), n, spec, SR))
    assert abs(r["hf"] - 1.0) < 1e-12 and abs(r["ht"] - 1.0) < 1e-12 and abs(r["h"] - 1.0) < 1e-12 and abs(r["bi"]) < 1e-9
    r = _named(S.indices(_seg(mean_power=np.full(257, 0.25)), np.full(n, 7.0), n, S.Spec(band=(1000.0, 3000.0)), SR))
    assert abs(r["hf"] - 1.0) < 1e-12
    # a constant-amplitude bin adds nothing to aci; a bin that alternates 0, 2 adds (n - 1) * 2 / (n * 1)
    amp, diff = np.ones(257), np.zeros(257)
    assert _named(S.indices(_seg(mean_amplitude=amp, abs_diff=diff), np.ones(n), n, spec, SR))["aci"] == 0.0
    diff[100] = 2.0 * (n - 1)
    assert abs(_named(S.indices(_seg(mean_amplitude=amp, abs_diff=diff), np.ones(n), n, spec, SR))["aci"] - 2.0 * (n - 1) / n) < 1e-12
    assert _named(S.indices(_seg(mean_amplitude=amp, abs_diff=diff), np.ones(n), n, S.Spec(band=(0.0, 3000.0)), SR))["aci"] == 0.0       # bin 100 is outside
    # bi: one bin 10 dB over the others in bio_band -> 10 dB * one bin width in kHz
    p = np.full(257, 1.0)
    p[100] = 10.0
    assert abs(_named(S.indices(_seg(mean_power=p), np.ones(n), n, spec, SR))["bi"] - 10.0 * 0.03125) < 1e-12
    # one frame: no temporal entropy
    assert math.isnan(_named(S.indices(_seg(mean_power=p), np.ones(1), 1, spec, SR))["ht"])
    # a non-finite frame: every column
    bad = dict(_seg(mean_power=p), nonfinite_frames=1)
    assert np.isnan(S.indices(bad, np.ones(n), n, spec, SR)).all()


def test_an_all_silent_segment():
    r = _named(S.indices(_seg(), np.zeros(5), 5, S.Spec(), SR))
    assert r["aci"] == 0.0 and r["bi"] == 0.0
    for name in ("ndsi", "hf", "ht", "adi", "aei", "h"):
        assert math.isnan(r[name]), name
    st = S.stats64(np.zeros(512 * 3, np.float32), 512, 3, -50.0)
    assert st["n_frames"].tolist() == [3] and (st["mean_power"] == 0).all() and (st["count_above"] == 0).all()
    assert np.array_equal(np.isnan(S.indices_of(st, S.Spec(), SR)[0]), [False, True, True, False, True, True, True, True])


def test_statistics_of_the_restatement_on_hand_worked_input():
    """A bin-centred tone switched on for the middle frame of three (hop 512): its bin holds P = (128 a)^2 there and 0 elsewhere."""
    t = np.arange(512)
    x = np.zeros(3 * 512, np.float32)
    x[512:1024] = (0.5 * np.cos(2 * np.pi * 64 * t / 512)).astype(np.float32)
    st = S.stats64(x, 512, 3, -20.0)
    assert st["n_frames"].tolist() == [3] and st["nonfinite_frames"].tolist() == [0]
    peak = (128 * 0.5) ** 2
    assert abs(st["mean_power"][0, 64] - peak / 3) < 1e-3 and abs(st["mean_amplitude"][0, 64] - 64.0 / 3) < 1e-4
    assert abs(st["abs_diff"][0, 64] - 128.0) < 1e-4 and st["count_above"][0, 64] == 1 and st["count_above"][0, 200] == 0
    assert abs(st["frame_power"][1] - 1.5 * peak) < 1e-2            # the window leaks a quarter into each neighbour bin
    two = S.stats64(x, 512, 2, -20.0)                               # the difference across a segment boundary is not counted
    assert two["n_frames"].tolist() == [2, 1] and abs(two["abs_diff"][0, 64] - 64.0) < 1e-4 and (two["abs_diff"][1] == 0).all()
    x[700] = np.inf
    bad = S.stats64(x, 512, 2, -20.0)
    assert bad["nonfinite_frames"].tolist() == [1, 0] and np.isnan(bad["mean_power"][0]).all() and np.isnan(bad["abs_diff"][0]).all()
    assert bad["count_above"][0].max() == 0 and not np.isnan(bad["mean_power"][1]).any()


# ------------------------------------------------------------------------------------------------------------- the count test's inputs
@pytest.mark.parametrize("hop", A.HOPS)
def test_count_allowances_stay_under_their_cap(hop):
    """What tests/test_gpu_soundscape.py's count test relies on, from the float64 reference and the float32 CPU chain alone: the cells close
    enough to the threshold to be allowed a different answer are at most 0.1 % of each input's cells."""
    synth = A.synthetic()
    for x, db in ((synth, -50.0), (synth[27200:49600], -60.0)):
        P64, P32 = A.frame_power64(x, hop), S.power32(x, hop)
        allow, bar = S.count_allowance(P64, P32, 64, db)
        frac = allow.sum() / P64.size
        print(f"hop {hop}, {len(x)} samples at {db} dBFS: bar {bar:.3e}, allowance {frac:.3e} of {P64.size} cells")
        assert frac <= 1e-3
    above = (A.frame_power64(synth[27200:49600], hop) > float(S.threshold(-60.0))).mean()
    assert 0.3 < above < 0.6                                            # the threshold sits inside the noise distribution
