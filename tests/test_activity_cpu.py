"""The band-limited activity gate without a GPU: the gate's validation, frame / window / bin planning against hand-worked cases, the
bindings, the argument checks of the four entry points, the new keywords, and the NumPy reference (tests/_activity_ref.py) on the
synthetic recording the GPU tests use -- including the margin those tests rely on."""
import inspect
import os
import re

import numpy as np
import pytest

import _activity_ref as A
import _recordings_ref as R
from avex_amd import _capi, activity, detection, recordings
from avex_amd.activity import ActivityGate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_refusals_and_defaults():
    g = ActivityGate([(2000, 8000)])
    assert (g.snr_db, g.min_active_frames, g.mode, g.hop, g.floor_percentile, g.min_floor_db) == (6.0, 2, "any", 256, 20.0, None)
    assert g.bands == ((2000.0, 8000.0),) and g.floor_min == np.float32(0.0) and g.ratio == np.float32(10.0 ** 0.6)
    assert ActivityGate([(0, 100)], min_floor_db=-60.0).floor_min == np.float32(1e-6)
    with pytest.raises(Exception):
        g.hop = 128                                                     # immutable
    for bad in ([], [(2000, 2000)], [(4000, 2000)], [(-1, 2000)], [(100, 200)] * 9, [(1, float("nan"))], [2000, 4000], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            ActivityGate(bad)
    for kw in (dict(hop=31), dict(hop=513), dict(hop=256.0), dict(hop=True), dict(floor_percentile=-0.1), dict(floor_percentile=100.5),
               dict(floor_percentile=float("nan")), dict(mode="most"), dict(min_active_frames=-1), dict(min_active_frames=1.5), dict(snr_db=float("inf")),
               dict(min_floor_db=float("nan"))):
        with pytest.raises(ValueError):
            ActivityGate([(2000, 4000)], **kw)
    assert ActivityGate([(2000, 4000)], hop=32).hop == 32 and ActivityGate([(2000, 4000)], hop=512, floor_percentile=100, min_active_frames=0).hop == 512
    with pytest.raises(ValueError):
        ActivityGate([(9000, 10000)]).bins(16000)                       # past Nyquist
    with pytest.raises(ValueError):
        ActivityGate([(2001, 2002)]).bins(16000)                        # between two bins: empty
    with pytest.raises(TypeError):
        activity.band_activity(None, "gate")


def test_bins():
    assert activity.band_bins(A.BANDS, 16000).tolist() == [[64, 128], [192, 256], [0, 257]] == [list(b) for b in A.bins(A.BANDS, 16000)]
    assert activity.band_bins([(0, 8000)], 16000).tolist() == [[0, 256]]                   # the Nyquist bin needs hi > 8000
    assert activity.band_bins([(0, 31.25), (31.25, 31.26), (7968.75, 9000)], 16000).tolist() == [[0, 1], [1, 2], [255, 257]]
    got = activity.band_bins([(2000, 4000), (0, 11025), (0, 11026), (10000, 20000)], 22050).tolist()
    assert got == [[47, 93], [0, 256], [0, 257], [233, 257]]            # 2000 * 512 / 22050 = 46.4, 4000 -> 92.9, 10000 -> 232.2
    assert got == [list(b) for b in A.bins([(2000, 4000), (0, 11025), (0, 11026), (10000, 20000)], 22050)]


def test_frame_and_window_planning():
    assert [activity.frame_count(n, 256) for n in (1, 511, 512, 513, 767, 768, 1024)] == [0, 0, 1, 1, 1, 2, 3]
    assert [activity.frame_count(n, 200) for n in (511, 512, 711, 712, 912, 16000)] == [0, 1, 1, 2, 3, 78]
    for hop in (32, 200, 256, 512):
        for n in (1, 511, 512, 513, 5000):
            assert activity.frame_count(n, hop) == A.n_frames_of(n, hop)
    # (start, valid, hop) -> (first frame, frames): frames lie wholly inside the window
    assert activity.window_frames(0, 16000, 200) == (0, 78)
    assert activity.window_frames(8000, 16000, 256) == (32, 60)         # ceil(31.25) = 32 .. floor(23488 / 256) = 91
    assert activity.window_frames(8000, 16000, 200) == (40, 78)         # 40 .. floor(23488 / 200) = 117
    assert activity.window_frames(96000, 123, 256) == (375, 0)          # a padded tail window shorter than a frame
    assert activity.window_frames(0, 511, 256) == (0, 0) and activity.window_frames(0, 512, 256) == (0, 1) and activity.window_frames(1, 512, 256) == (1, 0)
    assert activity.window_frames(256, 512, 256) == (1, 1) and activity.window_frames(255, 513, 256) == (1, 1)
    for hop in (200, 256):
        for s, v in ((0, 16000), (8000, 16000), (8001, 700), (96000, 123), (300, 511), (299, 1024)):
            fr = A.window_frames(s, v, hop)
            f_lo, n = activity.window_frames(s, v, hop)
            assert n == len(fr) and (n == 0 or fr == list(range(f_lo, f_lo + n))), (s, v, hop)
    g = ActivityGate([(0, 100)], floor_percentile=20.0)
    assert [g.floor_rank(n) for n in (0, 1, 2, 5, 6, 374)] == [0, 0, 0, 0, 1, 74] == [A.floor_rank(n, 20.0) for n in (0, 1, 2, 5, 6, 374)]
    assert ActivityGate([(0, 100)], floor_percentile=100).floor_rank(374) == 373 and ActivityGate([(0, 100)], floor_percentile=0).floor_rank(374) == 0


def test_tables():
    t = activity.tables()
    assert t.dtype == np.float32 and t.shape == (1536,) and np.array_equal(t[:512], A.hann())
    assert t[0] == 0.0 and t[256] == 1.0 and t[512] == 1.0 and t[513] == 0.0 and t[512 + 2 * 128] == np.float32(np.cos(np.pi / 2)) and t[512 + 2 * 128 + 1] == -1.0


def _declared(prefix):
    text = open(os.path.join(ROOT, "include", "avexhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_bindings(built_lib):
    assert _capi.header_abi_version() >= 21
    names = ["avexhip_activity_count", "avexhip_activity_floor", "avexhip_activity_frames", "avexhip_activity_select"]
    assert _declared("avexhip_activity_") == names == sorted(n for n in _capi.SYMBOLS if n.startswith("avexhip_activity_"))
    for n in names:
        assert hasattr(built_lib, n)
    import ctypes as C
    assert C.sizeof(_capi.ActivityRecording) == activity.RECORDING_DTYPE.itemsize == 32
    for (name, _), off in zip(_capi.ActivityRecording._fields_, (0, 8, 16, 24, 28)):
        assert getattr(_capi.ActivityRecording, name).offset == activity.RECORDING_DTYPE.fields[name][1] == off
    from avex_amd import build
    assert "activity.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["activity.hip"]
    text = open(os.path.join(ROOT, "include", "avexhip.h")).read()
    assert int(re.search(r"AVEXHIP_ACTIVITY_MAX_BANDS (\d+)", text).group(1)) == activity.MAX_BANDS
    assert int(re.search(r"AVEXHIP_ACTIVITY_MIN_HOP (\d+)", text).group(1)) == activity.MIN_HOP


def _rec_table(samples, hop, percentile=20.0):
    rec = np.zeros(len(samples), dtype=activity.RECORDING_DTYPE)
    frames = blocks = pos = 0
    for r, n in enumerate(samples):
        F = activity.frame_count(n, hop)
        rec[r] = (pos, n, frames, blocks, A.floor_rank(F, percentile))
        frames, blocks, pos = frames + F, blocks + (F + 7) // 8, (pos + n + 3) & ~3
    return rec, frames, pos


def test_argument_checks_need_no_gpu(built_lib):
    """Each entry point refuses a bad call before it touches the device; the pointers below are never dereferenced."""
    lib, fake = built_lib, 1 << 20
    rec, total, size = _rec_table([5000, 600], 256)
    assert total == 18 + 1
    bands = np.array([[64, 128], [0, 257]], dtype=np.int32)

    def frames(**kw):
        a = dict(wav=fake, size=size, rec=rec, rec_dev=fake, n_rec=2, hop=256, bands=bands, n_bands=2, tab=fake, total=total, out=fake)
        a.update(kw)
        return lib.avexhip_activity_frames(a["wav"], a["size"], a["rec"].ctypes.data if a["rec"] is not None else None, a["rec_dev"], a["n_rec"], a["hop"],
                                           a["bands"].ctypes.data, a["n_bands"], a["tab"], a["total"], a["out"], None)

    def bad_rec(**kw):
        t = rec.copy()
        for k, v in kw.items():
            t[k][1] = v
        return t

    for kw, word in ((dict(wav=None), "null"), (dict(rec=None), "null"), (dict(tab=None), "null"), (dict(out=None), "null"), (dict(wav=fake + 4), "aligned"),
                     (dict(rec_dev=fake + 4), "aligned"), (dict(hop=31), "hop"), (dict(hop=513), "hop"), (dict(n_bands=0), "n_bands"), (dict(n_bands=9), "n_bands"),
                     (dict(bands=np.array([[64, 64], [0, 257]], dtype=np.int32)), "band 0"), (dict(bands=np.array([[64, 128], [0, 258]], dtype=np.int32)), "band 1"),
                     (dict(bands=np.array([[-1, 128], [0, 257]], dtype=np.int32)), "band 0"), (dict(size=size - 1), "leave the buffer"), (dict(total=total + 1), "total_frames"),
                     (dict(n_rec=0), "n_rec"), (dict(rec=bad_rec(first_frame=17)), "first_frame"), (dict(rec=bad_rec(first_block=2)), "first_block"),
                     (dict(rec=bad_rec(floor_rank=1)), "floor_rank"), (dict(rec=bad_rec(n_samples=0)), "recording 1"), (dict(rec=bad_rec(base=-4)), "recording 1")):
        assert frames(**kw) == -1 and word in _capi.last_error(), (kw, _capi.last_error())

    def floor(**kw):
        a = dict(e=fake, total=total, rec=rec, rec_dev=fake, n_rec=2, hop=256, n_bands=2, fl=fake, bad=fake)
        a.update(kw)
        return lib.avexhip_activity_floor(a["e"], a["total"], a["rec"].ctypes.data, a["rec_dev"], a["n_rec"], a["hop"], a["n_bands"], a["fl"], a["bad"], None)

    for kw, word in ((dict(e=None), "null"), (dict(fl=None), "null"), (dict(bad=None), "null"), (dict(e=fake + 2), "aligned"), (dict(hop=0), "hop"),
                     (dict(n_bands=9), "n_bands"), (dict(total=total - 1), "total_frames"), (dict(rec=bad_rec(floor_rank=-1)), "floor_rank")):
        assert floor(**kw) == -1 and word in _capi.last_error(), (kw, _capi.last_error())

    win = np.zeros(3, dtype=recordings.WINDOW_DTYPE)
    win["base"], win["n_samples"], win["start"], win["valid"] = (0, 0, 5000), (5000, 5000, 600), (0, 4000, 0), (4000, 1000, 600)
    win_rec = np.array([0, 0, 1], dtype=np.int32)

    def count(**kw):
        a = dict(win=win, win_dev=fake, wr=win_rec, wr_dev=fake, n_win=3, rec=rec, rec_dev=fake, n_rec=2, hop=256, e=fake, total=total, fl=fake, n_bands=2,
                 floor_min=0.0, ratio=10.0, nf=fake, act=fake, mx=fake)
        a.update(kw)
        return lib.avexhip_activity_count(a["win"].ctypes.data, a["win_dev"], a["wr"].ctypes.data, a["wr_dev"], a["n_win"], a["rec"].ctypes.data, a["rec_dev"],
                                          a["n_rec"], a["hop"], a["e"], a["total"], a["fl"], a["n_bands"], a["floor_min"], a["ratio"], a["nf"], a["act"], a["mx"], None)

    def bad_win(row, **kw):
        t = win.copy()
        for k, v in kw.items():
            t[k][row] = v
        return t

    for kw, word in ((dict(win_dev=None), "null"), (dict(nf=None), "null"), (dict(e=None), "null"), (dict(win_dev=fake + 4), "aligned"), (dict(n_win=0), "n_win"),
                     (dict(ratio=float("nan")), "NaN"), (dict(floor_min=float("nan")), "NaN"), (dict(floor_min=-1.0), ">= 0"), (dict(hop=600), "hop"),
                     (dict(n_bands=0), "n_bands"), (dict(wr=np.array([0, 2, 1], dtype=np.int32)), "window 1"), (dict(wr=np.array([0, 0, 0], dtype=np.int32)), "window 2"),
                     (dict(win=bad_win(1, valid=1001)), "window 1"), (dict(win=bad_win(0, start=-1)), "window 0"), (dict(total=total + 8), "total_frames")):
        assert count(**kw) == -1 and word in _capi.last_error(), (kw, _capi.last_error())

    def select(**kw):
        a = dict(win=fake, e=fake, p=fake, act=fake, n_win=3, n_bands=2, k=2, mode=0, te=-np.inf, tp=-np.inf, kept=fake, cnt=fake)
        a.update(kw)
        return lib.avexhip_activity_select(a["win"], a["e"], a["p"], a["act"], a["n_win"], a["n_bands"], a["k"], a["mode"], a["te"], a["tp"], a["kept"], a["cnt"], None)

    for kw, word in ((dict(act=None), "null"), (dict(kept=None), "null"), (dict(e=fake + 4), "aligned"), (dict(n_win=0), "n_win"), (dict(n_bands=9), "n_bands"),
                     (dict(k=-1), "min_active_frames"), (dict(mode=2), "mode"), (dict(te=float("nan")), "NaN"), (dict(tp=float("nan")), "NaN")):
        assert select(**kw) == -1 and word in _capi.last_error(), (kw, _capi.last_error())


def test_new_keywords_default_to_none_and_come_last():
    for fn in (recordings.embed_recording, recordings.embed_recordings, detection.detect_events):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "activity" and p["activity"].default is None and p["activity"].kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    assert inspect.signature(recordings._embed).parameters["activity"].default is None
    import avex_amd
    assert avex_amd.ActivityGate is ActivityGate and avex_amd.band_activity is activity.band_activity
    assert "ActivityGate" in avex_amd.__all__ and "band_activity" in avex_amd.__all__


def test_reference_pieces_on_hand_made_numbers():
    e = np.array([3.0, 0.0, np.nan, 1.0, np.inf, 1.0, 2.0], dtype=np.float32)
    assert A.key_sorted(e)[:6].tolist() == [0.0, 1.0, 1.0, 2.0, 3.0, np.inf] and np.isnan(A.key_sorted(e)[6])     # NaN sorts above +inf
    assert A.noise_floor(e, 0.0) == 0.0 and A.noise_floor(e, 20.0) == 1.0 and A.noise_floor(e, 50.0) == 2.0 and np.isnan(A.noise_floor(e, 100.0))
    assert np.isnan(A.noise_floor(e[:0], 20.0)) and A.nonfinite_count(e) == 1
    assert A.threshold(np.float32(2.0), 10.0) == np.float32(20.0) and np.isnan(A.threshold(np.float32(np.nan), 10.0, -30.0))
    assert A.threshold(np.float32(0.0), 10.0, -30.0) == np.float32(np.float32(1e-3) * np.float32(10.0))
    # two bands over five frames at hop 256; windows (0, 1024): frames 0..2, (512, 1024): frames 2..4, (1280, 300): none
    energy = np.array([[1.0, 30.0, 1.0, np.nan, 10.0], [0.0, 0.0, 0.0, 0.0, 5.0]], dtype=np.float32)
    floors = np.array([1.0, 0.0], dtype=np.float32)
    nf, act, mx = A.window_stats(energy, floors, [0, 512, 1280], [1024, 1024, 300], 256, 10.0)
    assert nf.tolist() == [3, 3, 0] and act.tolist() == [[1, 0], [0, 1], [0, 0]]          # 10.0 > 10.0 is false; with a floor of 0 only silence is inactive
    assert mx[0].tolist() == [30.0, 0.0] and np.isnan(mx[1, 0]) and mx[1, 1] == 5.0 and mx[2].tolist() == [-np.inf, -np.inf]
    assert A.band_condition(act, 1, "any").tolist() == [True, True, False] and A.band_condition(act, 1, "all").tolist() == [False, False, False]
    assert A.band_condition(act, 0, "all").tolist() == [True, True, True]
    assert A.kept_list([0, 2], act, 1, "any") == [0] and A.kept_list([0, 1, 2], act, 0, "any") == [0, 1, 2]


@pytest.fixture(scope="module")
def synth():
    x = A.synthetic()
    kb = A.bins(A.BANDS, A.SR)
    return x, kb, {hop: A.band_energy(A.frame_power64(x, hop), kb).astype(np.float32) for hop in A.HOPS}


def test_reference_on_the_synthetic_recording(synth):
    x, kb, energy = synth
    assert x.dtype == np.float32 and len(x) == A.N_SYNTH == 96123 and abs(float(np.sqrt(np.mean(x[:16000].astype(np.float64) ** 2))) - 0.01) < 5e-4
    assert energy[256].shape == (3, 374) and energy[200].shape == (3, 479)
    starts, valids = R.plan(len(x), 16000, 8000)
    assert len(starts) == 13 and valids[-1] == 123
    for hop in A.HOPS:
        out = A.analyse(x, starts, valids, hop, kb, energy32=energy[hop])
        # the floor is the noise: Parseval, sum over 257 of 512 bins of |X|^2 ~ 512 sigma^2 sum w^2 / 2 = 512 * 1e-4 * 192 / 2 in the full band
        assert 0.5 * 4.9 < out["floor"][2] < 4.9 and out["floor"][0] < 0.4 * out["floor"][2] and out["nonfinite"] == 0
        act = out["active_frames"]
        assert out["n_frames"][-1] == 0 and out["n_frames"][0] == activity.window_frames(0, 16000, hop)[1]
        # 3 kHz bursts at 1.0-1.6 s and 3.2-3.25 s: windows 1..3 and 5, 6; 6.5 kHz at 4.5-5.2 s: windows 8..10
        assert [w for w in range(13) if act[w, 0] >= 2] == [1, 2, 3, 5, 6] and [w for w in range(13) if act[w, 1] >= 2] == [8, 9, 10]
        assert [w for w in range(13) if act[w, 2] >= 2] == [1, 2, 3, 5, 6, 8, 9, 10]
        level = R.select(*R.stats(x, starts, valids), valids)
        assert A.kept_list(level, act, 2, "any") == [1, 2, 3, 5, 6, 8, 9, 10] and A.kept_list(level, act, 2, "all") == []
        assert A.kept_list(level, act, 0, "all") == level == list(range(13))


def test_synthetic_recording_keeps_its_margin(synth):
    """What the end-to-end GPU test relies on: no frame energy within 5 % of its threshold, even with the floor one rank off."""
    _, _, energy = synth
    for hop in A.HOPS:
        closest = A.closest_approach(energy[hop], A.PERCENTILE, A.SNR_DB)
        print(f"hop {hop}: closest approach of an energy to its threshold {closest:.3f}")
        assert closest > A.MARGIN
