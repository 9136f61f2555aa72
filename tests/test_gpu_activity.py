"""The band-limited activity gate on the device: avex_amd.activity over csrc/activity.hip (avexhip_activity_frames / _floor / _count /
_select) against tests/_activity_ref.py.

Energies are compared with a float64 transform under a bar measured in the same test (8 x the deviation of a float32 CPU transform);
everything decided FROM the energies -- floors, counts, maxima, the kept list -- is compared bit for bit by feeding the device's own
energies to the NumPy restatement.
"""
import numpy as np
import pytest
import torch

import _activity_ref as A
import _recordings_ref as R
from avex_amd import activity, detection, recordings
from avex_amd.activity import ActivityGate

pytestmark = pytest.mark.gpu

W_LEN, W_HOP = 16000, 8000                # one-second windows every half second


def _ws(arrays, window_len=W_LEN, hop_len=W_HOP):
    return recordings.RecordingWindows([torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in arrays], A.SR, window_len, hop_len)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kept(sel):
    host = sel.cpu().numpy()
    return host[:int(host[-1])].tolist()


@pytest.fixture(scope="module")
def synth():
    return A.synthetic()


@pytest.fixture(scope="module")
def power64(synth):
    """The float64 reference of the synthetic recording, once per hop."""
    return {hop: A.frame_power64(synth, hop) for hop in A.HOPS}


# ------------------------------------------------------------------------------------------------------------- 1. energies against fp64
def _deviations(arrays, hop, bands, power=None):
    """(device deviation, float32 CPU deviation): max over recordings, bands and frames of |E - E64| / P_f."""
    gate = ActivityGate(bands, hop=hop)
    act = activity.band_activity(_ws(arrays), gate)
    kb = A.bins(bands, A.SR)
    got = act.frame_energy.cpu().numpy()
    assert got.shape == (len(bands), sum(A.n_frames_of(len(x), hop) for x in arrays)) and got.dtype == np.float32
    w = A.hann()
    dev = cpu = 0.0
    for r, x in enumerate(arrays):
        f0, f1 = act.frame_ranges[r]
        assert f1 - f0 == A.n_frames_of(len(x), hop)
        if f1 == f0:
            continue
        P = power[r] if power is not None else A.frame_power64(x, hop)
        total = P.sum(axis=1)
        frames = np.stack([x[f * hop:f * hop + 512] for f in range(f1 - f0)]).astype(np.float32)
        X = torch.fft.rfft(torch.from_numpy(frames * w))                                   # float32 product, float32 transform
        P32 = (X.real ** 2 + X.imag ** 2).numpy()
        for b, (lo, hi) in enumerate(kb):
            e64 = P[:, lo:hi].sum(axis=1)
            dev = max(dev, float(np.max(np.abs(got[b, f0:f1].astype(np.float64) - e64) / total)))
            cpu = max(cpu, float(np.max(np.abs(P32[:, lo:hi].sum(axis=1, dtype=np.float32).astype(np.float64) - e64) / total)))
    return dev, cpu


@pytest.mark.parametrize("hop", A.HOPS)
def test_energies_of_the_synthetic_recording(built_lib, synth, power64, hop):
    """374 frames at hop 256 (even), 479 at hop 200 (odd: the last frame has no partner; frame starts off the 16-byte grid)."""
    dev, cpu = _deviations([synth], hop, A.BANDS, [power64[hop]])
    print(f"hop {hop}: device deviation {dev:.3e}, float32 CPU deviation {cpu:.3e}")
    assert dev <= 8.0 * cpu


def test_energies_of_edge_bands_and_short_recordings(built_lib, synth):
    """Bin 0 alone, a band ending at bin 256, the Nyquist bin; recordings of 511 (no frame), 512 (one) and 40 001 samples in one call."""
    bands = ((0.0, 31.25), (7000.0, 8000.0), (7968.75, 9000.0), (0.0, 8001.0))
    assert A.bins(bands, A.SR) == [(0, 1), (224, 256), (255, 257), (0, 257)]
    arrays = [synth[1000:1511], synth[17000:17512], synth[15000:55001]]
    for hop in (200, 512):
        dev, cpu = _deviations(arrays, hop, bands)
        print(f"hop {hop}: device deviation {dev:.3e}, float32 CPU deviation {cpu:.3e}")
        assert dev <= 8.0 * cpu


# ------------------------------------------------------------------------------------------------------------- 2. exact properties
def test_a_silent_frame_beside_a_full_scale_one_is_plus_zero(built_lib):
    rng = np.random.default_rng(5)
    x = np.zeros(6 * 512, dtype=np.float32)
    x[0:512] = rng.uniform(-1.0, 1.0, 512)                              # pair (0, 1): loud, silent
    x[700:900] = -0.0
    x[3 * 512:4 * 512] = rng.choice([-1.0, 1.0], 512)                   # pair (2, 3): silent, loud (full scale)
    x[4 * 512 + 7] = 1.0                                                # pair (4, 5): an impulse, silence
    act = activity.band_activity(_ws([x], 1024, 1024), ActivityGate(A.BANDS, hop=512))
    e = act.frame_energy.cpu().numpy()
    assert e.shape == (3, 6) and (e[:, [0, 3, 4]] > 0).all()
    assert (_bits(e[:, [1, 2, 5]]) == 0).all()                          # +0, not a rounding residue and not -0


def test_bits_depend_on_the_recording_alone(built_lib, synth):
    x, short, other = synth[15000:55001], synth[:511], synth[60000:60700]
    gate = ActivityGate(A.BANDS, hop=200)
    alone = activity.band_activity(_ws([x]), gate)
    again = activity.band_activity(_ws([x]), gate)
    assert np.array_equal(_bits(alone.frame_energy), _bits(again.frame_energy)) and np.array_equal(_bits(alone.floor), _bits(again.floor))
    for arrays, r in (([short, x, other], 1), ([other, short, x], 2), ([x, other], 0)):
        among = activity.band_activity(_ws(arrays), gate)
        f0, f1 = among.frame_ranges[r]
        assert np.array_equal(_bits(among.frame_energy[:, f0:f1]), _bits(alone.frame_energy)), r
        assert np.array_equal(_bits(among.floor[r]), _bits(alone.floor[0]))


def test_nan_and_inf_stay_in_their_frames(built_lib, synth):
    x = synth[:8000].copy()
    x[1000], x[5003] = np.nan, -np.inf
    hop = 200
    act = activity.band_activity(_ws([x, synth[:4000]], 4000, 2000), ActivityGate(A.BANDS, hop=hop))
    e = act.frame_energy.cpu().numpy()
    F = A.n_frames_of(8000, hop)
    holds = np.array([any(f * hop <= i < f * hop + 512 for i in (1000, 5003)) for f in range(F)])
    assert holds.sum() == 6 and np.array_equal(np.isnan(e[:, :F]), np.broadcast_to(holds, (3, F))) and np.isfinite(e[:, F:]).all()
    assert act.nonfinite_frames.cpu().tolist() == [6, 0]
    clean = activity.band_activity(_ws([synth[:8000]], 4000, 2000), ActivityGate(A.BANDS, hop=hop)).frame_energy.cpu().numpy()
    far = np.array([not any(abs(f - g) <= 1 for g in np.flatnonzero(holds)) for f in range(F)])      # neither poisoned nor the partner of a poisoned frame
    assert np.array_equal(_bits(e[:, :F][:, far]), _bits(clean[:, far])) and np.isfinite(e[:, :F][:, ~holds]).all()


# ------------------------------------------------------------------------------------------------------------- 3. decisions, bit for bit
def _check_decisions(arrays, gate, window_len=W_LEN, hop_len=W_HOP, min_rms_db=None, min_peak_db=None):
    """Everything decided from the energies equals the restatement fed the device's own energies; returns the kept list."""
    ws = _ws(arrays, window_len, hop_len)
    act = activity.band_activity(ws, gate)
    kb = A.bins(gate.bands, A.SR)
    energy = act.frame_energy.cpu().numpy()
    floor, n_frames, active, mx = act.floor.cpu().numpy(), act.n_frames.cpu().numpy(), act.active_frames.cpu().numpy(), act.max_energy.cpu().numpy()
    level = []
    for r, x in enumerate(arrays):
        w0, w1 = ws.ranges[r]
        f0, f1 = act.frame_ranges[r]
        starts, valids = ws.starts[w0:w1], ws.valids[w0:w1]
        want = A.analyse(x, starts, valids, gate.hop, kb, gate.snr_db, gate.floor_percentile, gate.min_floor_db, energy32=energy[:, f0:f1])
        assert np.array_equal(_bits(floor[r]), _bits(want["floor"])), (r, floor[r], want["floor"])
        assert int(act.nonfinite_frames[r]) == want["nonfinite"]
        assert np.array_equal(n_frames[w0:w1], want["n_frames"]) and np.array_equal(active[w0:w1], want["active_frames"]), r
        assert np.array_equal(_bits(mx[w0:w1]), _bits(want["max_energy"])), r
        level += [w0 + w for w in R.select(*R.stats(x, starts, valids), valids, *R.thresholds(min_rms_db, min_peak_db))]
    kept = _kept(act.select(min_rms_db, min_peak_db))
    assert kept == A.kept_list(level, active, gate.min_active_frames, gate.mode)
    return ws, act, kept


def _tied():
    """Period 256 = the hop: whole stretches of identical frames, so the floor's rank falls among equal energies."""
    rng = np.random.default_rng(11)
    period = (0.05 * rng.standard_normal(256)).astype(np.float32)
    x = np.tile(period, 40)
    x[3000:3600] += (0.5 * np.sin(2 * np.pi * 3000.0 * np.arange(600) / A.SR)).astype(np.float32)
    x[7000:7800] += (0.5 * np.sin(2 * np.pi * 6500.0 * np.arange(800) / A.SR)).astype(np.float32)
    return x


@pytest.mark.parametrize("mode", ["any", "all"])
@pytest.mark.parametrize("percentile", [0.0, 20.0, 100.0])
def test_decisions_on_the_synthetic_recording(built_lib, synth, percentile, mode):
    bad = synth[:9000].copy()
    bad[4321] = np.nan                                                  # NaN frames sort above everything: the floor at p = 100 is a NaN
    arrays = [synth, synth[:511], bad]
    for hop in A.HOPS:
        gate = ActivityGate(A.BANDS, snr_db=A.SNR_DB, floor_percentile=percentile, hop=hop, mode=mode, min_active_frames=2)
        _check_decisions(arrays, gate, min_rms_db=-45.0)


def test_decisions_with_ties_at_the_floor(built_lib):
    x = _tied()
    for percentile in (0.0, 20.0, 50.0, 100.0):
        ws, act, _ = _check_decisions([x], ActivityGate(A.BANDS, snr_db=6.0, floor_percentile=percentile, hop=256, min_active_frames=1), 2048, 1024)
    e = act.frame_energy.cpu().numpy()
    assert len(np.unique(_bits(e[2]))) < e.shape[1] // 2                # the ties are there


def test_decisions_with_a_floor_of_zero_and_a_floor_bound(built_lib, synth):
    x = np.zeros(20000, dtype=np.float32)
    x[5000:5600] = synth[16000:16600]                                   # a piece of the 3 kHz burst in digital silence
    x[12000:12050] = 1e-4 * synth[:50]                                  # and something faint
    gate = ActivityGate(A.BANDS, snr_db=10.0, hop=256, min_active_frames=1)
    ws, act, kept = _check_decisions([x], gate, 4000, 2000)
    assert (_bits(act.floor) == 0).all()                                # the floor is +0: every frame that is not silent is active
    e = act.frame_energy.cpu().numpy()
    assert act.active_frames[:, 2].sum().item() > 0 and kept == [1, 2, 5, 6]
    for w in range(ws.n_windows):
        f, n = activity.window_frames(int(ws.starts[w]), int(ws.valids[w]), 256)
        assert int(act.active_frames[w, 2]) == int((e[2, f:f + n] > 0).sum())
    bound = ActivityGate(A.BANDS, snr_db=10.0, hop=256, min_active_frames=1, min_floor_db=-30.0)
    _, _, kept = _check_decisions([x], bound, 4000, 2000)
    assert kept == [1, 2]                                               # the faint piece no longer counts
    _check_decisions([x], ActivityGate(A.BANDS, snr_db=10.0, hop=256, min_active_frames=1, mode="all", min_floor_db=-30.0), 4000, 2000)


def test_without_a_frame_count_the_list_is_the_level_gate(built_lib, synth):
    x = synth.copy()
    x[24000:56000] *= np.float32(0.01)
    for mode in ("any", "all"):
        ws, act, kept = _check_decisions([x, synth[:511]], ActivityGate(A.BANDS, hop=200, min_active_frames=0, mode=mode), min_rms_db=-50.0, min_peak_db=-40.0)
        assert kept == _kept(ws.select(-50.0, -40.0)) and torch.equal(act.select(), ws.select())      # (past the count a list is not written)
        assert 0 < len(kept) < ws.n_windows


def test_decisions_over_more_windows_than_one_pass_of_the_select(built_lib):
    """Nine recordings cut into windows of 768 samples (two frames each at hop 256, none in a recording's short last window): more than
    1 024 windows, so the kept list is written in a second pass behind the first one's count."""
    arrays = [A.synthetic(seed=r) for r in range(9)]
    arrays[3] = arrays[3] * np.float32(0.001)                           # bursts at -70 dBFS: the level gate drops the whole recording
    for mode in ("any", "all"):
        gate = ActivityGate(A.BANDS, snr_db=A.SNR_DB, hop=256, mode=mode, min_active_frames=1)
        ws, act, kept = _check_decisions(arrays, gate, 768, 768, min_rms_db=-45.0)
        assert ws.n_windows > 1024 and not any(ws.ranges[3][0] <= k < ws.ranges[3][1] for k in kept)
        if mode == "any":
            assert sum(k < 1024 for k in kept) > 64 and sum(k >= 1024 for k in kept) > 8 and len(kept) < ws.n_windows // 2


# ------------------------------------------------------------------------------------------------------------- 4. end to end
class _StandIn:
    """What recordings._embed asks of a model; its embedding is four exact facts about the window."""

    def __init__(self):
        self._hook_layers = []

    def register_hooks_for_layers(self, layers):
        self._hook_layers = list(layers)

    def ensure_hooks_registered(self):
        pass

    def extract_embeddings(self, batch, aggregation="mean"):
        wav, mask = batch["raw_wav"], batch["padding_mask"]
        return torch.stack([wav[:, 0], wav[:, 100], wav.abs().amax(dim=1), (~mask).sum(dim=1).to(torch.float32)], dim=1)


def _reference_kept(x, hop, power, min_active_frames=2, mode="any"):
    starts, valids = R.plan(len(x), W_LEN, W_HOP)
    kb = A.bins(A.BANDS, A.SR)
    out = A.analyse(x, starts, valids, hop, kb, energy32=A.band_energy(power, kb).astype(np.float32))
    return A.kept_list(R.select(*R.stats(x, starts, valids), valids), out["active_frames"], min_active_frames, mode), out


@pytest.mark.parametrize("hop", A.HOPS)
def test_the_gate_keeps_what_the_fp64_reference_keeps(built_lib, synth, power64, hop):
    """No exclusions: the synthetic recording keeps every energy 5 % away from its threshold (tests/test_activity_cpu.py asserts it)."""
    want, ref = _reference_kept(synth, hop, power64[hop])
    assert want == [1, 2, 3, 5, 6, 8, 9, 10]
    gate = ActivityGate(A.BANDS, snr_db=A.SNR_DB, floor_percentile=A.PERCENTILE, hop=hop)
    act = activity.band_activity(_ws([synth]), gate)
    assert _kept(act.select()) == want
    assert np.array_equal(act.active_frames.cpu().numpy(), ref["active_frames"]) and np.array_equal(act.n_frames.cpu().numpy(), ref["n_frames"])
    assert np.allclose(act.floor.cpu().numpy()[0], ref["floor"], rtol=1e-4)

    model = _StandIn()
    r = recordings.embed_recordings(model, [synth], 1.0, 0.5, activity=gate)[0]
    ws = recordings.windows(synth, 1.0, 0.5)
    wav, mask = ws.batch(np.asarray(want))
    assert r["window_index"].tolist() == want and torch.equal(r["embeddings"], model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}))
    assert r["kept"].tolist() == [w in want for w in range(13)]
    assert torch.equal(r["active_frames"], act.active_frames) and np.array_equal(_bits(r["floor"]), _bits(act.floor[0]))
    one = recordings.embed_recording(model, synth, 1.0, 0.5, activity=gate, min_peak_db=-20.0)
    assert one["window_index"].tolist() == want and set(one) == set(r)
    none_kept = recordings.embed_recording(model, synth, 1.0, 0.5, activity=ActivityGate(A.BANDS, snr_db=60.0, hop=hop))
    assert none_kept["window_index"].tolist() == [] and none_kept["embeddings"].shape == (0,)


def test_without_a_gate_nothing_changes(built_lib, synth):
    model = _StandIn()
    keys = {"embeddings", "window_index", "start_s", "end_s", "kept", "rms_db", "peak_db"}
    ws = recordings.windows(synth, 1.0, 0.5)
    wav, mask = ws.batch(0, ws.n_windows)
    for kw in ({}, {"activity": None}):
        r = recordings.embed_recording(model, synth, 1.0, 0.5, **kw)
        assert set(r) == keys and torch.equal(r["embeddings"], model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}))
        assert r["window_index"].tolist() == list(range(13)) and torch.equal(r["rms_db"], ws._device_db()[0])
    gated = recordings.embed_recording(model, synth, 1.0, 0.5, min_rms_db=-35.0, activity=None)
    assert set(gated) == keys and gated["window_index"].tolist() == _kept(ws.select(-35.0, None))


def test_detect_events_takes_the_gate(built_lib, synth):
    gate = ActivityGate(A.BANDS, snr_db=A.SNR_DB, hop=256)
    out = detection.detect_events(_StandIn(), lambda e: e[:, 2:3], [synth], 1.0, 0.5, on=0.2, activity=gate, return_scores=True)
    rows = out["row_of_window"].cpu().tolist()
    assert [w for w, r in enumerate(rows) if r >= 0] == [1, 2, 3, 5, 6, 8, 9, 10] and out["scores"].shape == (8, 1)
    assert int(out["count"]) == 3 and out["first"].tolist() == [1, 5, 8] and out["last"].tolist() == [3, 6, 10]
