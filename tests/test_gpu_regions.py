"""Sound-event regions on the device: avex_amd.regions over csrc/regions.hip against tests/_regions_ref.py.

The labelling is integer work and is compared exactly: every column of label_cells with the NumPy union-find of the restatement, on the
smallest masks that can go wrong (run, word, ballot, prefix-block and recording boundaries, every reach, long chains).  find_regions'
mask is compared with a float64 chain under the rule of test_gpu_soundscape.py's count test: the cells closer to the threshold than
bar * P_f, bar = 8 x the largest deviation of a float32 CPU chain, may differ, and they may be at most 1 % of all cells; the rows are
then those of the restatement fed the device's own mask, exactly.
"""
import csv

import numpy as np
import pytest
import torch

import _activity_ref as A
import _measure_ref as M
import _regions_ref as R
import _soundscape_ref as S
from avex_amd import measurements, recordings, regions, soundscape
from avex_amd.annotations import Annotations
from avex_amd.measurements import MeasureSpec
from avex_amd.regions import RegionSpec
from avex_amd.soundscape import IndexSpec

pytestmark = pytest.mark.gpu

SR = A.SR
EDGE_BINS = (0, 31, 32, 63, 64, 255, 256)                               # word and ballot boundaries


def _ws(arrays):
    return recordings.RecordingWindows([torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in arrays], SR, 16000, 16000)


def _cols(r, names=regions.COLUMNS):
    return {k: r[k].cpu().numpy() for k in names}


def _same(got, want, what=""):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])


def _label(mask, frames, reach=(1, 1), **filters):
    """label_cells of a host mask against the restatement: the packed mask, n_found and every column."""
    r = regions.label_cells(torch.from_numpy(mask).cuda(), frames, reach, **filters)
    want, n_found, _ = R.label(mask, frames, reach, **filters)
    assert np.array_equal(R.unpack(r.cells.cpu().numpy()), mask) and r.cells.shape == (len(mask), 9) and r.cells.dtype == torch.int32
    assert int(r.n_found) == n_found and r.n_cells == int(mask.sum()), (int(r.n_found), n_found)
    assert r.frame_offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist() and r.nonfinite_frames.cpu().tolist() == [0] * len(frames)
    _same(_cols(r), want, (frames, reach, filters))
    return r, want, n_found


def _random(F, density, seed):
    return np.random.default_rng(seed).random((F, 257)) < density


# ------------------------------------------------------------------------------------------------------------- 1. label_cells, exactly
@pytest.mark.parametrize("F,density", [(1, 0.3), (64, 0.3), (65, 0.3), (130, 0.3), (2100, 0.004)])
def test_frame_counts(built_lib, F, density):
    """1, 64 and 65 frames (a run of the cells kernel), 130 (three), 2 100 with a sparse mask (the 1 024-frame prefix block, twice)."""
    _, want, n = _label(_random(F, density, F), [F])
    assert n > 1 and len(want["n_cells"]) == n


@pytest.mark.parametrize("density", [0.02, 0.3, 0.6])
def test_random_masks(built_lib, density):
    _, want, n = _label(_random(70, density, 7), [70])
    assert n >= 1 and want["n_cells"].sum() == _random(70, density, 7).sum()
    _label(_random(70, density, 8), [30, 40])


@pytest.mark.parametrize("reach", [(1, 1), (0, 1), (1, 0), (0, 0), (2, 3), (4, 8)])
def test_every_reach(built_lib, reach):
    mask = _random(40, 0.03, 11)
    mask[10:20, 100:110] = np.random.default_rng(12).random((10, 10)) < 0.5
    _, _, n_one = _label(mask, [40], reach)
    _, _, n_two = _label(mask, [17, 23], reach)
    assert n_two >= n_one
    if reach == (0, 0):
        assert n_one == mask.sum()


def test_recordings_stay_apart(built_lib):
    """The last frame of a recording and the first of the next set in the same bins: separate regions; a recording without a frame in
    between; one that holds nothing at the start and at the end."""
    mask = np.zeros((9, 257), bool)
    mask[:, 40:50] = True
    mask[:, 256] = True
    for frames, reach in (([4, 5], (1, 1)), ([3, 3, 3], (1, 1)), ([4, 0, 5], (1, 1)), ([0, 4, 0, 0, 5, 0], (4, 8)), ([1] * 9, (2, 2))):
        _, want, n = _label(mask, frames, reach)
        held = [r for r, f in enumerate(frames) if f]
        assert n == 2 * len(held) and want["recording"].tolist() == [r for r in held for _ in range(2)]
        assert want["first_frame"].tolist() == [0] * n and want["last_frame"].tolist() == [frames[r] - 1 for r in held for _ in range(2)]
    _, want, n = _label(mask, [9], (1, 1))
    assert n == 2 and want["n_cells"].tolist() == [90, 9] and want["n_frames"].tolist() == [9, 9] and want["n_bins"].tolist() == [10, 1]


def test_word_and_ballot_boundaries(built_lib):
    """Bins 0, 31, 32, 63, 64, 255 and 256 alone and in pairs, every case in a frame of its own with empty frames around it."""
    cases = [(b,) for b in EDGE_BINS] + [(a, b) for i, a in enumerate(EDGE_BINS) for b in EDGE_BINS[i + 1:]]
    mask = np.zeros((3 * len(cases), 257), bool)
    for i, bins in enumerate(cases):
        mask[3 * i + 1, list(bins)] = True
    for reach in ((1, 1), (0, 1), (1, 0), (2, 8)):
        _, want, n = _label(mask, [len(mask)], reach)
        joined = sum(1 for c in cases if len(c) == 2 and c[1] - c[0] <= reach[1])
        assert n == len(EDGE_BINS) + 2 * 21 - joined and (want["n_frames"] == 1).all()
    # the same pairs one frame apart: bin a in frame f, bin b in frame f + 1
    pairs = [c for c in cases if len(c) == 2] + [(b, a) for a, b in cases[len(EDGE_BINS):]]
    mask = np.zeros((4 * len(pairs), 257), bool)
    for i, (a, b) in enumerate(pairs):
        mask[4 * i + 1, a], mask[4 * i + 2, b] = True, True
    for reach in ((1, 1), (1, 0), (2, 8)):
        _, want, n = _label(mask, [len(mask)], reach)
        assert n == 2 * len(pairs) - sum(1 for a, b in pairs if abs(a - b) <= reach[1])


def test_no_wrap_from_bin_256_into_the_next_frame(built_lib):
    mask = np.zeros((10, 257), bool)
    mask[1, 256] = mask[2, 0] = True
    mask[7, 255:] = mask[8, :2] = True
    for reach in ((1, 1), (4, 8)):
        _, want, n = _label(mask, [10], reach)
        assert n == 4 and want["low_bin"].tolist() == [256, 0, 255, 0] and want["high_bin"].tolist() == [256, 0, 256, 1]


def test_checkerboard_full_and_empty(built_lib):
    f, k = np.indices((66, 257))
    board = (f + k) % 2 == 0
    _, want, n = _label(board, [66])
    assert n == 1 and want["n_cells"].tolist() == [int(board.sum())] and want["n_bins"].tolist() == [257]
    for reach in ((0, 0), (1, 0), (0, 1)):
        assert _label(board, [66], reach)[2] == board.sum()           # every cell a region of its own
    _, want, n = _label(board, [66], (0, 2))
    assert n == 66 and (want["n_frames"] == 1).all()
    full = np.ones((130, 257), bool)
    _, want, n = _label(full, [130])
    assert n == 1 and want["n_cells"].tolist() == [257 * 130] and want["last_frame"].tolist() == [129]
    _, want, n = _label(full, [130], (0, 0), min_cells=2)
    assert n == 257 * 130 and len(want["n_cells"]) == 0
    for F in (0, 1, 70):                                                # an empty mask: zero rows, nothing launched past the count
        r, want, n = _label(np.zeros((F, 257), bool), [F])
        assert n == 0 and all(r[k].shape == (0,) and r[k].dtype == torch.int32 for k in regions.COLUMNS)
    assert _label(np.zeros((0, 257), bool), [0, 0])[2] == 0


def test_long_chains(built_lib):
    """A serpentine 200 frames long -- rows of set bins in every other frame, joined at alternating ends -- whose smallest cell is one
    end of the path, and a comb whose teeth join only in the last frame."""
    snake = np.zeros((200, 257), bool)
    snake[0::2, 10:251] = True
    snake[1::4, 250] = True
    snake[3::4, 10] = True
    snake[199] = False
    _, want, n = _label(snake, [200], (1, 1))
    assert n == 1 and want["first_frame"].tolist() == [0] and want["last_frame"].tolist() == [198] and want["n_cells"].tolist() == [int(snake.sum())]
    assert _label(snake, [200], (0, 1))[2] == 100 + 99                  # without the frame links: the rows and the joints
    _label(snake, [120, 80], (1, 1))
    up = snake[::-1].copy()                                             # and with the links the other way round
    assert _label(up, [200], (1, 1))[2] == 1
    comb = np.zeros((70, 257), bool)
    comb[:, 0::4] = True
    comb[69] = True
    _, want, n = _label(comb, [70])
    assert n == 1 and want["n_cells"].tolist() == [69 * 65 + 257]
    assert _label(comb[:69], [69])[2] == 65
    assert _label(comb[::-1].copy(), [70])[2] == 1


@pytest.mark.parametrize("filters", [dict(min_cells=5), dict(min_frames=3), dict(min_bins=4), dict(max_frames=2), dict(min_cells=3, min_frames=2, min_bins=2, max_frames=6),
                                      dict(min_cells=1, min_frames=1, min_bins=1, max_frames=None), dict(min_cells=100000)])
def test_filters(built_lib, filters):
    mask = _random(1100, 0.06, 21)
    _, want, n = _label(mask, [600, 500], (1, 1), **filters)
    all_, n_all, _ = R.label(mask, [600, 500])
    assert n == n_all and len(want["n_cells"]) <= n
    if filters.get("max_frames", 1) is None:
        assert len(want["n_cells"]) == n
    elif "min_cells" in filters and filters["min_cells"] == 5 and len(filters) == 1:
        assert 0 < len(want["n_cells"]) < n and want["n_cells"].tolist() == [c for c in all_["n_cells"] if c >= 5]


# ------------------------------------------------------------------------------------------------------------- 2. determinism, company
def test_repeat_calls_and_company(built_lib):
    a, b, c = _random(70, 0.2, 31), _random(33, 0.5, 32), _random(129, 0.05, 33)
    alone = _cols(regions.label_cells(torch.from_numpy(a).cuda(), [70], (2, 2)))
    for _ in range(3):
        _same(_cols(regions.label_cells(torch.from_numpy(a).cuda(), [70], (2, 2))), alone, "repeat")
    for masks, at in (((a, b, c), 0), ((b, c, a), 2), ((c, a, b), 1), ((c, b, a), 2)):
        frames = [len(m) for m in masks]
        r = regions.label_cells(torch.from_numpy(np.concatenate(masks)).cuda(), frames, (2, 2))
        got = _cols(r)
        mine = got["recording"] == at
        assert mine.sum() == len(alone["recording"])
        _same({k: v[mine] for k, v in got.items() if k != "recording"}, {k: v for k, v in alone.items() if k != "recording"}, (at,))
        assert np.array_equal(r.cells.cpu().numpy()[sum(frames[:at]):sum(frames[:at + 1])], regions.label_cells(torch.from_numpy(a).cuda(), [70]).cells.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------- 3. find_regions
@pytest.fixture(scope="module")
def synth():
    return A.synthetic()


_POWER = {}


def _power(x, hop):
    """(float64 reference, float32 CPU chain) of a recording, computed once."""
    key = (hash(x.tobytes()), len(x), hop)
    if key not in _POWER:
        _POWER[key] = (A.frame_power64(x, hop), S.power32(x, hop))
    return _POWER[key]


def _noise(ws, hop):
    return measurements.noise_spectrum(soundscape.spectral_stats(ws, IndexSpec(hop=hop, segment_s=1.0)))


def _excused(P64, P32, thr):
    """(the cells close enough to the threshold to be decided either way, bar): |P64 - thr| <= bar * P_f, bar = 8 x max |P32 - P64| / P_f."""
    pf = P64.sum(axis=1, keepdims=True)
    bar = 8.0 * float(np.max(np.abs(P32.astype(np.float64) - P64) / pf))
    return np.abs(P64 - thr.astype(np.float64)[None, :]) <= bar * pf, bar


@pytest.mark.parametrize("hop", [256, 200, 128])
@pytest.mark.parametrize("snr_db", [10.0, 15.0])
def test_find_regions_on_the_synthetic_recording(built_lib, synth, hop, snr_db):
    """(a) the device's mask equals P64 > thr except at excused cells, at most 1 % of all; (b) the rows are the restatement's over the
    device's own mask, exactly; (c) at hop 256 and 15 dB no cell is excused (asserted first) and the whole result is the float64 chain's.
    Measured on an MI355X: see DESIGN.md 4.11m."""
    ws = _ws([synth])
    noise = _noise(ws, hop)
    spec = RegionSpec(hop=hop, snr_db=snr_db)
    r = regions.find_regions(ws, spec, noise_power=noise)
    P64, P32 = _power(synth, hop)
    F = len(P64)
    thr = R.threshold(noise.cpu().numpy(), snr_db, None, 1)
    assert np.array_equal(spec.threshold(noise, 1, noise.device).cpu().numpy(), thr) and np.isfinite(thr).all()
    mask = R.unpack(r.cells.cpu().numpy())
    ref = R.mask_of_power(P64, thr[0])
    near, bar = _excused(P64, P32, thr[0])
    differ = mask != ref
    print(f"hop {hop}, {snr_db} dB: bar {bar:.3e}, {int(near.sum())} of {ref.size} cells excused, the device differs at {int(differ.sum())}; {int(mask.sum())} cells set, "
          f"{int(r.n_found)} regions")
    assert near.sum() <= 0.01 * ref.size                                # the cap
    assert not (differ & ~near).any()                                   # (a)
    want, n_found, _ = R.label(mask, [F])                               # (b)
    assert mask.shape == (F, 257) and int(r.n_found) == n_found and r.nonfinite_frames.cpu().tolist() == [0] and (r.sr, r.hop) == (SR, hop)
    _same(_cols(r), want)
    _same(_cols(r, regions.FLOAT_COLUMNS), R.derived(want, hop, SR))
    assert ref[:, 96].sum() > 30 and mask[:, 96].sum() > 30             # the 3 kHz bursts stand out
    big = int(np.argmax(want["n_cells"]))                               # the largest region is one of the long bursts, at 3 kHz or at 6.5 kHz
    assert want["n_frames"][big] > 10 and any(want["low_bin"][big] <= k <= want["high_bin"][big] for k in (96, 208))
    if (hop, snr_db) == (256, 15.0):                                    # (c)
        assert near.sum() == 0
        end_to_end, n64, _ = R.label(ref, [F])
        assert n64 == n_found
        _same(_cols(r), end_to_end)


def test_silence_nan_samples_and_nan_noise(built_lib, synth):
    hop = 200
    quiet = np.zeros(20000, np.float32)
    quiet[3000:3300] = -0.0
    x = synth[:40001].copy()
    x[6000], x[15003] = np.nan, -np.inf
    short = synth[:3000]
    ws = _ws([quiet, x, short, synth[:40001]])
    noise = _noise(ws, hop)
    nh = noise.cpu().numpy()
    assert (nh[0] == 0).all() and np.isnan(nh[2]).all() and np.isfinite(nh[1]).all() and np.isfinite(nh[3]).all()      # 3 000 samples hold no full segment
    r = regions.find_regions(ws, RegionSpec(hop=hop, snr_db=10.0), noise_power=noise)
    mask, off = R.unpack(r.cells.cpu().numpy()), r.frame_offsets.cpu().numpy()
    frames = [A.n_frames_of(n, hop) for n in (20000, 40001, 3000, 40001)]
    assert off.tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist()
    assert not mask[off[0]:off[1]].any()                                # silence: +0 is not above a threshold of 0
    bad = [f for f in range(frames[1]) if any(f * hop <= i < f * hop + 512 for i in (6000, 15003))]
    assert r.nonfinite_frames.cpu().tolist() == [0, len(bad), 0, 0] and len(bad) == 6
    assert not mask[off[1] + np.asarray(bad)].any() and mask[off[1]:off[2]].any()      # no cell in a NaN frame
    assert not mask[off[2]:off[3]].any() and mask[off[3]:off[4]].any()  # a NaN noise row: no cell, and no region, for that recording only
    got = _cols(r)
    assert set(got["recording"].tolist()) == {1, 3}
    _same(got, R.label(mask, frames)[0])
    clean = regions.find_regions(_ws([synth[:40001]]), RegionSpec(hop=hop, snr_db=10.0), noise_power=noise[3:4])
    mine = got["recording"] == 3
    _same({k: v[mine] for k, v in got.items() if k != "recording"}, {k: v for k, v in _cols(clean).items() if k != "recording"})
    same_frames = np.setdiff1d(np.arange(frames[1]), bad)               # the frames that avoid the samples: the bits of a clean run (the noise rows differ: own threshold)
    own = regions.find_regions(_ws([synth[:40001]]), RegionSpec(hop=hop, snr_db=10.0), noise_power=noise[1:2])
    assert np.array_equal(R.unpack(own.cells.cpu().numpy())[same_frames], mask[off[1] + same_frames])
    floor_only = regions.find_regions(_ws([quiet]), RegionSpec(hop=hop, min_db=-90.0))
    assert int(floor_only.n_found) == 0 and floor_only.n_cells == 0 and floor_only["recording"].shape == (0,) and floor_only["begin_s"].shape == (0,)


def test_band_and_min_db_alone(built_lib, synth):
    hop = 256
    ws = _ws([synth])
    noise = _noise(ws, hop)
    whole = R.unpack(regions.find_regions(ws, RegionSpec(hop=hop), noise_power=noise).cells.cpu().numpy())
    spec = RegionSpec(hop=hop, band=(2000.0, 4000.0))
    assert spec.bins(SR) == (64, 128)
    r = regions.find_regions(ws, spec, noise_power=noise)
    banded = R.unpack(r.cells.cpu().numpy())
    assert banded[:, 64:128].any() and not banded[:, :64].any() and not banded[:, 128:].any() and np.array_equal(banded[:, 64:128], whole[:, 64:128])
    _same(_cols(r), R.label(banded, [len(banded)])[0])
    assert (r["low_bin"] >= 64).all() and (r["high_bin"] < 128).all()
    # min_db alone, without a noise spectrum: the float64 chain outside the excused cells
    P64, P32 = _power(synth, hop)
    spec = RegionSpec(hop=hop, min_db=-40.0, reach=(2, 2), min_cells=4)
    r = regions.find_regions(ws, spec)
    thr = R.threshold(None, spec.snr_db, -40.0, 1)[0]
    mask = R.unpack(r.cells.cpu().numpy())
    near, _ = _excused(P64, P32, thr)
    assert near.sum() <= 0.01 * near.size and not ((mask != R.mask_of_power(P64, thr)) & ~near).any() and 0 < mask.sum() < 0.2 * mask.size
    _same(_cols(r), R.label(mask, [len(mask)], (2, 2), min_cells=4)[0])
    with pytest.raises(ValueError):
        regions.find_regions(ws, RegionSpec(hop=hop))                  # neither a noise spectrum nor min_db
    with pytest.raises(ValueError):
        regions.find_regions(ws, RegionSpec(hop=hop), noise_power=torch.zeros(2, 257, device="cuda"))


@pytest.mark.parametrize("hop", [32, 160, 512])
def test_cells_are_the_soundscape_kernels_bits(built_lib, synth, hop):
    """regions_cells_kernel and soundscape_stats_kernel run one text for P[f, k] (frame_power.h) and both apply the strict P > thr with
    thr = fl32(16384 * 10^(d / 10)): with one frame per segment, count_above IS the mask, cell for cell, and a frame that holds a NaN
    is all clear in both."""
    d = -60.0                                                           # the float32 CPU chain sets 42.9 % / 43.2 % / 42.1 % of the cells at hops 32 / 160 / 512
    x = synth[15000:31001].copy()                                       # 1 s: 485 / 97 / 31 frames
    x[7000] = np.nan
    ws = _ws([x])
    r = regions.find_regions(ws, RegionSpec(hop=hop, min_db=d))
    stats = soundscape.spectral_stats(ws, IndexSpec(hop=hop, segment_s=hop / SR, db_threshold=d))
    assert np.float32(RegionSpec(hop=hop, min_db=d).floor) == np.float32(IndexSpec(hop=hop, segment_s=hop / SR, db_threshold=d).threshold)
    mask, count = R.unpack(r.cells.cpu().numpy()), stats.count_above.cpu().numpy()
    F = A.n_frames_of(len(x), hop)
    assert mask.shape == count.shape == (F, 257) and np.array_equal(mask, count == 1) and np.isin(count, (0, 1)).all()
    bad = [f for f in range(F) if f * hop <= 7000 < f * hop + 512]
    assert len(bad) == {32: 16, 160: 3, 512: 1}[hop] and not mask[bad].any() and not count[bad].any()
    assert r.nonfinite_frames.cpu().tolist() == [len(bad)] and np.flatnonzero(stats.nonfinite_frames.cpu().numpy()).tolist() == bad
    assert 0.05 <= mask.mean() <= 0.95


def test_find_regions_in_company(built_lib, synth):
    """A recording's rows are the same bits alone and with two others, in both orders, apart from the recording column."""
    hop = 128
    x, loud, other = synth[15000:55001], np.random.default_rng(5).choice([-1.0, 1.0], 30000).astype(np.float32), synth[:20000]
    noise = {id(a): _noise(_ws([a]), hop) for a in (x, loud, other)}
    spec = RegionSpec(hop=hop, snr_db=8.0, reach=(1, 2))
    alone = _cols(regions.find_regions(_ws([x]), spec, noise_power=noise[id(x)]))
    assert len(alone["recording"]) > 10
    for arrays, at in (([x, loud, other], 0), ([other, loud, x], 2), ([loud, x, other], 1), ([x], 0)):
        got = _cols(regions.find_regions(_ws(arrays), spec, noise_power=torch.cat([noise[id(a)] for a in arrays])))
        mine = got["recording"] == at
        _same({k: v[mine] for k, v in got.items() if k != "recording"}, {k: v for k, v in alone.items() if k != "recording"}, at)


# ------------------------------------------------------------------------------------------------------------- 4. measure_boxes(bins=...)
def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("hop", A.HOPS)
def test_measure_boxes_with_bins(built_lib, synth, hop):
    """The boxes and bands of _measure_ref, each band given as the box's own bins: the statistics against float64 under 8 x the float32
    CPU chain's deviation, the measurements against the restatement fed the device's statistics (integers equal, floats to 1e-9), the
    decisions against the float64 chain -- the comparison rules of test_gpu_measurements.py -- and the bits of the same boxes measured
    through a band per class."""
    ws = _ws([synth])
    boxes = [(a, b, lo, hi) for a, b in M.BOXES for lo, hi in M.BANDS]
    s0, s1 = [b[0] for b in boxes], [b[1] for b in boxes]
    bins = np.asarray([[b[2], b[3]] for b in boxes], dtype=np.int64)
    m = measurements.measure_boxes(ws, [0] * len(boxes), s0, s1, MeasureSpec(hop=hop), bins=bins)
    h = {k: v.cpu().numpy() for k, v in m.items()}
    P64, P32 = _power(synth, hop)
    for e, (a, b, lo, hi) in enumerate(boxes):
        f0, n = M.event_frames(a, b, hop, len(synth))
        env = h["envelope"][h["frame_offsets"][e]:h["frame_offsets"][e + 1]]
        assert (h["first_frame"][e], h["n_frames"][e]) == (f0, n) and len(env) == n
        assert (_bits(h["spectrum"][e, :lo]) == 0).all() and (_bits(h["spectrum"][e, hi:]) == 0).all()
        ref_s, ref_e, bad = M.stats_of_power(P64, f0, n, lo, hi)
        cpu_s, cpu_e, _ = M.stats_of_power(P32, f0, n, lo, hi)
        dev, cpu = M.deviations(h["spectrum"][e], env, ref_s, ref_e, P64, f0, n), M.deviations(cpu_s, cpu_e, ref_s, ref_e, P64, f0, n)
        assert bad == 0 and dev[0] <= 8.0 * cpu[0] and dev[1] <= 8.0 * cpu[1], (boxes[e], dev, cpu)
        want = M.measure(h["spectrum"][e], env, int(h["nonfinite"][e]), f0, lo, hi, hop, SR)
        for k in M.INTS:
            assert h[k][e] == want[k], (boxes[e], k)
        for k in M.FLOATS:
            g, w = float(h[k][e]), float(want[k])
            assert (np.isnan(g) and np.isnan(w)) or g == w or abs(g - w) <= 1e-9 * abs(w), (boxes[e], k, g, w)
        box64 = M.measure_box(P64, a, b, lo, hi, hop, SR, len(synth))
        for k in ("n_frames", "low_bin", "centre_bin", "high_bin", "peak_bin", "low_frame", "centre_frame", "high_frame"):
            assert h[k][e] == box64[k], (boxes[e], k)
    per_class = measurements.measure_boxes(ws, [0] * len(boxes), s0, s1, MeasureSpec(hop=hop, band=[(0.0, 8001.0), (2000.0, 8000.0), (1000.0, 4001.0)]),
                                           class_id=[e % 3 for e in range(len(boxes))])
    for k in m:
        assert np.array_equal(_bits(m[k]), _bits(per_class[k])), k
    # bins=None: every code path is the one without the keyword
    plain, none = measurements.measure_boxes(ws, [0, 0], [0, 16000], [96123, 25600], MeasureSpec(hop=hop, band=(2000.0, 8000.0))), \
        measurements.measure_boxes(ws, [0, 0], [0, 16000], [96123, 25600], MeasureSpec(hop=hop, band=(2000.0, 8000.0)), bins=None)
    assert set(plain) == set(none)
    for k in plain:
        assert np.array_equal(_bits(plain[k]), _bits(none[k])), k
    padded = measurements.measure_boxes(ws, [0, -1], [0, 0], [9000, 0], MeasureSpec(hop=hop), bins=[[5, 9], [0, 0]])       # a padded row's pair is not read
    assert padded["n_frames"].cpu().tolist()[1] == -1 and int(padded["low_bin"][0]) >= 5 and int(padded["high_bin"][0]) < 9
    for bad in ([[0, 258]], [[5, 5]], [[-1, 4]], [[7, 3]], [0, 257], [[0.0, 257.0]], [[0, 257], [0, 257]]):
        with pytest.raises(ValueError):
            measurements.measure_boxes(ws, [0], [0], [9000], MeasureSpec(hop=hop), bins=bad)


def test_regions_measure_and_raven_round_trip(built_lib, synth, tmp_path):
    hop = 200
    arrays = [synth, synth[15000:55001]]
    ws = _ws(arrays)
    noise = _noise(ws, hop)
    r = regions.find_regions(ws, RegionSpec(hop=hop, snr_db=12.0, reach=(2, 2), min_cells=6), noise_power=noise)
    E = len(r["recording"])
    assert E >= 4 and set(r["recording"].cpu().tolist()) == {0, 1}
    rec, s0, s1, bins = r.boxes()
    want = R.boxes(_cols(r), hop)
    for g, w in zip((rec, s0, s1, bins), want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    f0, n = measurements.event_frames(s0, s1, hop, np.asarray([len(arrays[i]) for i in rec]))
    assert np.array_equal(f0, r["first_frame"].cpu().numpy()) and np.array_equal(f0 + n - 1, r["last_frame"].cpu().numpy())
    m = r.measure(ws, noise_power=noise)
    assert np.array_equal(m["n_frames"].cpu().numpy(), r["n_frames"].cpu().numpy()) and np.array_equal(m["first_frame"].cpu().numpy(), f0) and m.hop == hop
    assert (m["low_bin"] >= r["low_bin"]).all() and (m["high_bin"] <= r["high_bin"]).all() and (m["nonfinite"] == 0).all()
    assert (m["low_frame"] >= r["first_frame"]).all() and (m["high_frame"] <= r["last_frame"]).all() and (m["energy"] > 0).all()
    events, meas = r.as_events(), r.as_measurements()
    assert (events["class_id"] == 0).all() and np.array_equal(events["peak"], r["n_cells"].cpu().numpy().astype(np.float64)) and meas.sr == SR
    paths = []
    for i in range(2):
        paths.append(tmp_path / f"rec{i}.txt")
        rows = measurements.write_raven(paths[-1], events, meas, recording=i)
        assert rows == int((r["recording"] == i).sum()) > 0
    back = Annotations.from_raven(paths, class_column="Species")
    assert np.array_equal(back.recording, r["recording"].cpu().numpy()) and (back.class_id == 0).all()
    assert np.array_equal(back.start_s, r["begin_s"].cpu().numpy()) and np.array_equal(back.end_s, r["end_s"].cpu().numpy())
    low, high, score = [], [], []
    for p in paths:
        with open(p, newline="", encoding="utf-8") as f:
            for row in csv.DictReader(f, delimiter="\t"):
                low.append(float(row["Low Freq (Hz)"]))
                high.append(float(row["High Freq (Hz)"]))
                score.append(float(row["Score"]))
    assert np.array_equal(low, r["low_hz"].cpu().numpy()) and np.array_equal(high, r["high_hz"].cpu().numpy()) and np.array_equal(score, events["peak"])
    bare = regions.label_cells(torch.zeros(4, 257, dtype=torch.bool, device="cuda"), [4])
    for call in (bare.boxes, bare.as_measurements, lambda: bare.measure(ws)):
        with pytest.raises(ValueError):
            call()
