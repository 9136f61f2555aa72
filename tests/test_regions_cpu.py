"""Sound-event regions without a GPU: the ABI number, RegionSpec's validation, the bindings, the argument checks that refuse before any
launch, the NumPy restatement (tests/_regions_ref.py) against scipy.ndimage.label and hand-worked masks, the boxes' arithmetic against
measurements.event_frames, and the condition test (c) of tests/test_gpu_regions.py relies on, asserted from the CPU chains alone."""
import math

import numpy as np
import pytest

import _activity_ref as A
import _regions_ref as R
import _soundscape_ref as S
from avex_amd import _capi, measurements, regions
from avex_amd.regions import RegionSpec

SR = A.SR


def test_abi_version_and_bindings(built_lib):
    assert _capi.header_abi_version() >= 25
    for name in ("avexhip_regions_workspace_bytes", "avexhip_regions_cells", "avexhip_regions_pack", "avexhip_regions_count", "avexhip_regions_label",
                 "avexhip_regions_rows"):
        assert name in _capi.SYMBOLS and hasattr(built_lib, name)
    W = built_lib.avexhip_regions_workspace_bytes
    assert W(0, 0) == 0 and W(-1, 0) == 0 and W(0, -1) == 0 and W(1 << 31, 0) == 0 and W(0, 1 << 31) == 0
    assert W(1000, 0) == 4096 + 256 and W(2100, 0) == 8448 + 256                 # one integer per frame, one per 1 024 frames, in steps of 256 bytes
    assert W(0, 1000) == 9 * 4096 + 256 and W(2100, 1000) == W(2100, 0) + W(0, 1000)      # nine integers per set cell
    assert regions.RECORDING_DTYPE.itemsize == 32 and regions.RULE_DTYPE.itemsize == 24
    assert regions.COLUMNS == R.COLUMNS
    import avex_amd
    for name in ("RegionSpec", "find_regions", "label_cells"):
        assert name in avex_amd.__all__ and getattr(avex_amd, name) is getattr(regions, name)


def test_struct_layouts_match_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{root}/include/avexhip.h"', "int main(void){"]
    want = {}
    for cname, dt in (("avexhip_regions_recording", regions.RECORDING_DTYPE), ("avexhip_regions_rule", regions.RULE_DTYPE)):
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
    s = RegionSpec()
    assert (s.hop, s.band, s.snr_db, s.min_db, s.reach, s.min_cells, s.min_frames, s.min_bins, s.max_frames) == (128, None, 10.0, None, (1, 1), 1, 1, 1, None)
    assert s.ratio == np.float32(10.0) == R.ratio32(10.0) and s.floor == 0.0 and s.bins(SR) == (0, 257)
    assert s.rule.tolist() == [(1, 1, 1, 1, 1, -1)]
    t = RegionSpec(hop=200, band=(1000, 4001), snr_db=6, min_db=-50.0, reach=[2, 3], min_cells=4, min_frames=np.int64(2), min_bins=3, max_frames=9)
    assert t.bins(SR) == (32, 129) and t.reach == (2, 3) and t.rule.tolist() == [(2, 3, 4, 2, 3, 9)] and isinstance(t.min_frames, int)
    assert t.floor == np.float32(16384.0 * 1e-5) == S.threshold(-50.0) == R.floor32(-50.0) and t.ratio == R.ratio32(6)
    with pytest.raises(Exception):
        s.hop = 256                                                     # immutable
    for kw in (dict(hop=31), dict(hop=513), dict(hop=128.0), dict(hop=True), dict(band=(2000, 2000)), dict(band=(-1, 5)), dict(band=2000), dict(band=(1, 2, 3)),
               dict(snr_db=math.nan), dict(snr_db="loud"), dict(min_db=math.inf), dict(min_db="quiet"), dict(reach=(5, 1)), dict(reach=(1, 9)), dict(reach=(-1, 1)),
               dict(reach=(1, -1)), dict(reach=1), dict(reach=(1, 1, 1)), dict(reach=(1.0, 1)), dict(reach=(True, 1)), dict(min_cells=0), dict(min_frames=0),
               dict(min_bins=0), dict(min_bins=1.5), dict(max_frames=0), dict(max_frames=-1), dict(min_cells=1 << 31)):
        with pytest.raises(ValueError):
            RegionSpec(**kw)
    with pytest.raises(ValueError):
        RegionSpec(band=(9000, 10000)).bins(SR)                         # past Nyquist
    with pytest.raises(ValueError):
        RegionSpec(band=(2001, 2002)).bins(SR)                          # between two bins
    with pytest.raises(TypeError):
        regions.find_regions(None, "spec")
    import torch
    with pytest.raises(ValueError):
        RegionSpec().threshold(None, 2, torch.device("cpu"))            # neither noise nor min_db
    with pytest.raises(ValueError):
        RegionSpec().threshold(torch.zeros(3, 257), 2, torch.device("cpu"))
    for kw in (dict(reach=(5, 0)), dict(min_cells=0), dict(max_frames=0)):
        with pytest.raises(ValueError):
            regions.label_cells(torch.zeros(4, 257, dtype=torch.bool), [4], **kw)
    for mask, frames in ((torch.zeros(4, 257), [4]), (torch.zeros(4, 256, dtype=torch.bool), [4]), (torch.zeros(4, 257, dtype=torch.bool), [3]),
                         (torch.zeros(4, 257, dtype=torch.bool), [5, -1]), (torch.zeros(4, 257, dtype=torch.bool), [])):
        with pytest.raises(ValueError):
            regions.label_cells(mask, frames)


def test_threshold_construction():
    import torch
    noise = np.array([[1.0] * 257, [np.nan] * 257, [1e-9] * 257], dtype=np.float32)
    noise[0, 5], noise[0, 6] = 3.3, 1e30
    for snr_db, min_db in ((10.0, None), (6.0, -50.0), (15.0, -90.0), (400.0, -50.0)):
        spec = RegionSpec(snr_db=snr_db, min_db=min_db)
        got = spec.threshold(torch.from_numpy(noise), 3, torch.device("cpu")).numpy()
        want = R.threshold(noise, snr_db, min_db, 3)
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), (snr_db, min_db)      # (a NaN's payload is not part of the result)
        assert np.isnan(got[1]).all()                                    # a NaN noise row stays NaN: no cell of that recording can be set
        if min_db is not None and snr_db < 100.0:
            assert (got[2] == spec.floor).all()                          # the floor holds where the noise is below it
        if snr_db > 100.0:
            assert np.isinf(got[0]).all() and np.isinf(got[2]).all()      # a ratio past float32: +inf, no cell
    only = RegionSpec(min_db=-40.0).threshold(None, 2, torch.device("cpu")).numpy()
    assert np.array_equal(only, R.threshold(None, 10.0, -40.0, 2)) and (only == np.float32(16384.0 * 1e-4)).all()
    assert (R.mask_of_power(np.array([[np.nan] * 257, [5.0] * 257]), np.full(257, 4.0, np.float32), 3, 200).sum(axis=1) == [0, 197]).all()
    assert not R.mask_of_power(np.full((2, 257), 4.0), np.full(257, 4.0, np.float32)).any()                       # strict
    assert not R.mask_of_power(np.full((2, 257), 4.0), np.full(257, np.nan, np.float32)).any()


def _recs(n_samples, hop):
    rec = np.zeros(len(n_samples), dtype=regions.RECORDING_DTYPE)
    rec["n_samples"] = n_samples
    rec["base"] = np.cumsum([0] + [(v + 3) & ~3 for v in n_samples[:-1]])
    f = np.asarray([A.n_frames_of(v, hop) for v in n_samples], dtype=np.int64)
    runs = (f + 63) // 64
    rec["first_frame"], rec["first_run"] = np.cumsum(f) - f, np.cumsum(runs) - runs
    return rec, int(f.sum())


def test_entry_points_refuse_before_any_launch(built_lib):
    """Every refusal comes from the host checks: the pointers below are never read on the device (this test runs without one)."""
    L = built_lib
    rec, F = _recs([40001, 511, 6000], 200)
    assert F == 198 + 28
    host, dev, buf = rec.ctypes.data, 0x1000, 0x10000
    total = int(rec["base"][-1] + rec["n_samples"][-1])

    def cells(**kw):
        a = dict(wav=buf, wav_samples=total, host=host, dev=dev, n_rec=3, hop=200, lo=0, hi=257, thr=buf, tab=buf, F=F, cells=buf, bad=buf)
        a.update(kw)
        return L.avexhip_regions_cells(a["wav"], a["wav_samples"], a["host"], a["dev"], a["n_rec"], a["hop"], a["lo"], a["hi"], a["thr"], a["tab"], a["F"], a["cells"],
                                       a["bad"], None)

    for kw in (dict(wav=None), dict(tab=None), dict(thr=None), dict(host=None), dict(dev=None), dict(bad=None), dict(wav=buf + 4), dict(tab=buf + 8), dict(thr=buf + 2),
               dict(dev=dev + 4), dict(cells=buf + 2), dict(bad=buf + 1), dict(hop=31), dict(hop=513), dict(hop=256), dict(n_rec=0), dict(wav_samples=total - 1),
               dict(wav_samples=0), dict(F=F + 1), dict(F=F - 1), dict(lo=-1), dict(lo=5, hi=5), dict(hi=258), dict(lo=200, hi=100)):
        assert cells(**kw) == -1 and _capi.last_error().startswith("regions_cells:"), kw
    for field, value in (("first_frame", 1), ("first_run", 2), ("n_samples", 0), ("base", -4), ("base", total)):      # a table that is not in order; a recording that leaves the buffer
        bad = rec.copy()
        bad[field][1] = value
        assert cells(host=bad.ctypes.data) == -1, field
    huge = np.zeros(2, dtype=regions.RECORDING_DTYPE)                    # 2^31 frames: two recordings of 2^30 frames at hop 32
    n = (1 << 30) * 32 + 480
    huge["n_samples"], huge["base"], huge["first_frame"], huge["first_run"] = n, [0, n], [0, 1 << 30], [0, 1 << 24]
    assert L.avexhip_regions_cells(buf, 2 * n, huge.ctypes.data, dev, 2, 32, 0, 257, buf, buf, 1 << 31, buf, buf, None) == -1 and "2^31" in _capi.last_error()

    rule = RegionSpec().rule
    offsets = np.array([0, 198, 198, 226], dtype=np.int64)
    fb, cb = L.avexhip_regions_workspace_bytes(F, 0), L.avexhip_regions_workspace_bytes(0, 1000)

    def label(**kw):
        a = dict(cells=buf, host=offsets, dev=dev, n_rec=3, F=F, n=1000, rule=rule, fws=buf, fb=fb, cws=buf, cb=cb, counts=buf)
        a.update(kw)
        return L.avexhip_regions_label(a["cells"], a["host"].ctypes.data if a["host"] is not None else None, a["dev"], a["n_rec"], a["F"], a["n"],
                                       a["rule"].ctypes.data if a["rule"] is not None else None, a["fws"], a["fb"], a["cws"], a["cb"], a["counts"], None)

    def changed(field, value):
        r = rule.copy()
        r[field][0] = value
        return r

    for kw in (dict(cells=None), dict(host=None), dict(dev=None), dict(dev=dev + 4), dict(rule=None), dict(fws=None), dict(cws=None), dict(counts=None),
               dict(counts=buf + 4), dict(cells=buf + 2), dict(n_rec=0), dict(F=F + 1), dict(n=-1), dict(n=F * 257 + 1),
               dict(host=np.array([0, 198, 197, 226], dtype=np.int64)), dict(host=np.array([1, 198, 198, 226], dtype=np.int64)),
               dict(host=np.array([0, 198, 198, 1 << 31], dtype=np.int64), F=1 << 31), dict(rule=changed("rt", 5)), dict(rule=changed("rt", -1)),
               dict(rule=changed("rk", 9)), dict(rule=changed("min_cells", 0)), dict(rule=changed("min_frames", 0)), dict(rule=changed("min_bins", -3)),
               dict(rule=changed("max_frames", 0)), dict(rule=changed("max_frames", -2))):
        assert label(**kw) == -1 and _capi.last_error().startswith("regions_label:"), kw
    assert label(fb=fb - 1) == -4 and label(cb=cb - 1) == -4
    big = np.array([0, (1 << 31) - 1], dtype=np.int64)                   # 2^31 set cells: refused after the first read, the threshold named as the remedy
    assert label(host=big, n_rec=1, F=(1 << 31) - 1, n=1 << 31) == -1 and "threshold" in _capi.last_error() and "2^31" in _capi.last_error()

    assert L.avexhip_regions_count(None, F, buf, fb, buf, None) == -1 and L.avexhip_regions_count(buf, F, None, fb, buf, None) == -1
    assert L.avexhip_regions_count(buf, F, buf, fb, None, None) == -1 and L.avexhip_regions_count(buf, 1 << 31, buf, fb, buf, None) == -1
    assert L.avexhip_regions_count(buf, F, buf, fb - 1, buf, None) == -4
    assert L.avexhip_regions_pack(None, F, buf, None) == -1 and L.avexhip_regions_pack(buf, F, None, None) == -1 and L.avexhip_regions_pack(buf, -1, buf, None) == -1
    assert L.avexhip_regions_pack(None, 0, None, None) == 0             # no frame: success, and nothing to launch
    rows = lambda **kw: L.avexhip_regions_rows(kw.get("n", 1000), kw.get("kept", 10), kw.get("rule", rule).ctypes.data, kw.get("cws", buf), kw.get("cb", cb),
                                               kw.get("counts", buf), kw.get("rows", buf), None)
    for kw in (dict(n=-1), dict(n=1 << 31), dict(kept=-1), dict(kept=1001), dict(cws=None), dict(counts=None), dict(rows=None), dict(rows=buf + 2),
               dict(rule=changed("rk", 9))):
        assert rows(**kw) == -1 and _capi.last_error().startswith("regions_rows:"), kw
    assert rows(cb=cb - 1) == -4 and rows(kept=0, cws=None, rows=None) == 0


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_scipy_label_for_reach_1_1():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for trial in range(30):
        F = int(rng.integers(1, 40))
        mask = rng.random((F, 257)) < (0.02, 0.3, 0.6)[trial % 3]
        cols, n_found, labels = R.label(mask, [F])
        want, n = ndimage.label(mask, structure=np.ones((3, 3)))
        assert n_found == n and np.array_equal(labels, want), trial
        sl = ndimage.find_objects(want)
        assert cols["first_frame"].tolist() == [s[0].start for s in sl] and cols["last_frame"].tolist() == [s[0].stop - 1 for s in sl]
        assert cols["low_bin"].tolist() == [s[1].start for s in sl] and cols["high_bin"].tolist() == [s[1].stop - 1 for s in sl]
        assert cols["n_cells"].tolist() == np.bincount(want.ravel())[1:].tolist() and (cols["recording"] == 0).all()
        four = ndimage.label(mask, structure=[[0, 0, 0], [1, 1, 1], [0, 0, 0]])[0]          # reach (0, 1): along the bins of one frame
        assert np.array_equal(R.label(mask, [F], reach=(0, 1))[2], four)
        assert R.label(mask, [F], reach=(0, 0))[1] == int(mask.sum())


def test_restatement_on_hand_worked_masks():
    m = np.zeros((5, 257), bool)
    m[0, 256] = m[1, 0] = True                                           # no wrap from bin 256 into the next frame's bin 0
    m[2, 10] = m[3, 12] = True                                           # two bins apart
    m[4, 100:104] = True
    cols, n, _ = R.label(m, [5])
    assert n == 5 and cols["n_cells"].tolist() == [1, 1, 1, 1, 4] and cols["low_bin"].tolist() == [256, 0, 10, 12, 100] and cols["n_bins"].tolist() == [1, 1, 1, 1, 4]
    cols, n, _ = R.label(m, [5], reach=(1, 2))
    assert n == 4 and cols["n_cells"].tolist() == [1, 1, 2, 4] and cols["first_frame"].tolist() == [0, 1, 2, 4] and cols["n_frames"].tolist() == [1, 1, 2, 1]
    cols, n, _ = R.label(m, [5], reach=(1, 2), min_cells=2)
    assert n == 4 and cols["n_cells"].tolist() == [2, 4]
    cols, n, _ = R.label(m, [5], reach=(1, 2), min_frames=2)
    assert cols["n_cells"].tolist() == [2]
    cols, n, _ = R.label(m, [5], reach=(1, 2), min_bins=2, max_frames=1)
    assert cols["n_cells"].tolist() == [4] and cols["recording"].dtype == np.int32
    # the same bins in the last frame of one recording and the first of the next: two regions; a recording without a frame in between
    m = np.zeros((4, 257), bool)
    m[1, 30:40] = m[2, 30:40] = True
    assert R.label(m, [4])[1] == 1
    cols, n, _ = R.label(m, [2, 0, 2])
    assert n == 2 and cols["recording"].tolist() == [0, 2] and cols["first_frame"].tolist() == [1, 0] and cols["last_frame"].tolist() == [1, 0]
    words = np.zeros((2, 9), np.int32)
    words[0, 0], words[0, 1], words[1, 8], words[1, 7] = 1, -(1 << 31), 1, 1 << 30
    got = R.unpack(words)
    assert np.argwhere(got).tolist() == [[0, 0], [0, 63], [1, 254], [1, 256]]


def test_boxes_give_back_the_regions_frames():
    rng = np.random.default_rng(1)
    for hop in (32, 128, 200, 256, 512):
        n_samples = 512 + 999 * hop + int(rng.integers(0, hop))
        first = rng.integers(0, 1000, 200)
        last = np.minimum(first + rng.integers(0, 50, 200), 999)
        cols = {"recording": np.zeros(200, np.int32), "first_frame": first.astype(np.int32), "last_frame": last.astype(np.int32),
                "low_bin": np.full(200, 3, np.int32), "high_bin": np.full(200, 256, np.int32)}
        rec, s0, s1, bins = R.boxes(cols, hop)
        f0, n = measurements.event_frames(s0, s1, hop, n_samples)
        assert np.array_equal(f0, first) and np.array_equal(f0 + n - 1, last) and (bins == [3, 257]).all() and (s1 <= n_samples).all()
        d = R.derived(cols, hop, SR)
        assert np.array_equal(d["begin_s"], s0 / SR) and np.array_equal(d["end_s"], s1 / SR) and (d["bandwidth_hz"] == 254 * SR / 512).all()


def test_regions_boxes_arithmetic():
    import torch
    r = regions.Regions({"recording": torch.tensor([0, 2], dtype=torch.int32), "first_frame": torch.tensor([3, 0], dtype=torch.int32),
                         "last_frame": torch.tensor([3, 77], dtype=torch.int32), "low_bin": torch.tensor([0, 100], dtype=torch.int32),
                         "high_bin": torch.tensor([256, 100], dtype=torch.int32)})
    r.sr, r.hop = SR, 200
    rec, s0, s1, bins = r.boxes()
    assert rec.tolist() == [0, 2] and s0.tolist() == [600, 0] and s1.tolist() == [1112, 77 * 200 + 512] and bins.tolist() == [[0, 257], [100, 101]]
    f0, n = measurements.event_frames(s0, s1, 200, 40001)
    assert f0.tolist() == [3, 0] and n.tolist() == [1, 78]
    r.sr = r.hop = None
    with pytest.raises(ValueError):
        r.boxes()


# ------------------------------------------------------------------------------------------------------------- the mask tests' inputs
def _noise32(P32, hop):
    """The noise spectrum of one recording from the float32 CPU chain: the minimum over its full one-second segments (the segments of
    tests/test_gpu_regions.py) of the float32 mean power."""
    seg = int(round(1.0 * SR / hop))
    st = S.stats_of_power(P32, seg, -50.0)
    full = [g for g in range(len(st["n_frames"])) if st["n_frames"][g] == seg and st["nonfinite_frames"][g] == 0]
    return np.min(st["mean_power"][full], axis=0).astype(np.float32)


@pytest.mark.parametrize("hop", (256, 200, 128))
def test_excused_cells_stay_under_their_cap(hop):
    """What tests/test_gpu_regions.py's mask test relies on, from the float64 reference and the float32 CPU chain alone: the cells close
    enough to the threshold to be excused are at most 1 % of all cells, and at hop 256 and 15 dB there is none that the float32 chain
    decides differently."""
    x = A.synthetic()
    P64, P32 = A.frame_power64(x, hop), S.power32(x, hop)
    noise = _noise32(P32, hop)
    pf = P64.sum(axis=1, keepdims=True)
    bar = 8.0 * float(np.max(np.abs(P32.astype(np.float64) - P64) / pf))
    for snr_db in (10.0, 15.0, 6.0):
        thr = R.threshold(noise[None], snr_db, None, 1)[0]
        near = np.abs(P64 - thr.astype(np.float64)[None, :]) <= bar * pf
        differ = R.mask_of_power(P64, thr) != R.mask_of_power(P32, thr)
        print(f"hop {hop}, {snr_db} dB: bar {bar:.3e}, {int(near.sum())} of {P64.size} cells excused, the float32 chain differs at {int(differ.sum())}")
        assert near.sum() <= 0.01 * P64.size and not (differ & ~near).any()
        if (hop, snr_db) == (256, 15.0):
            assert near.sum() == 0                                       # the configuration of the end-to-end test
