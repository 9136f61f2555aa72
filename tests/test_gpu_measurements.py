"""Event measurements on the device: avex_amd.measurements over csrc/measure.hip (avexhip_measure_frames / _reduce) against
tests/_measure_ref.py.

The fp32 statistics have yardsticks that exist: with the full band they are, bit for bit, what avex_amd.soundscape computes over the same
frames.  Against a float64 chain they stand under bars measured in the same test: 8 x the same deviation of a float32 CPU chain
(torch.fft.rfft of the fp32 product, fp32 |.|^2 and sums), the rule of test_gpu_soundscape.py.  The measurements, fp64 on the device, are
compared with the restatement fed the device's own statistics: integers equal, floats to 1e-9.  What must be exact -- silence,
independence of an event from its company -- is compared bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import _activity_ref as A
import _measure_ref as M
import _soundscape_ref as S
from avex_amd import _capi, detection, measurements, recordings, soundscape
from avex_amd.base_model import ModelBase
from avex_amd.measurements import MeasureSpec
from avex_amd.soundscape import IndexSpec

pytestmark = pytest.mark.gpu

SR = A.SR
BANDS_HZ = ((0.0, 8001.0), (2000.0, 8000.0), (1000.0, 4001.0))          # M.BANDS in Hz at 16 kHz (asserted in test_measurements_cpu.py)
ROWS = M.INTS + M.FLOATS + ("spectrum", "first_frame", "box_begin_s", "box_end_s")      # one row per event; "recording" follows the company


def _ws(arrays):
    return recordings.RecordingWindows([torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in arrays], SR, 16000, 16000)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _host(m):
    return {k: v.cpu().numpy() for k, v in m.items()}


def _event(h, e):
    """Event e of a host result: its row of every column and its envelope."""
    out = {k: h[k][e] for k in ROWS}
    out["envelope"] = h["envelope"][h["frame_offsets"][e]:h["frame_offsets"][e + 1]]
    return out


def _same_bits(a, b, what=""):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, a[k], b[k])


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


def _check(arrays, boxes, hop, bands_hz=BANDS_HZ, p=0.9, noise=None, stats=True, per_box=True):
    """boxes: (recording, s0, s1, band number).  Every box's statistics against float64 under the 8 x float32-CPU-chain bar -- each box
    under its own, or (``per_box=False``) the largest deviation over the boxes under 8 x the largest of the CPU chain, the way
    test_gpu_soundscape.py pools its recordings: the maximum over one frame and one bin is a single rounding error, which can be 0 --
    then every measurement against the restatement fed the device's own statistics.  Returns the host result and the (device, float32
    CPU) deviation pairs of spectrum and envelope with the largest ratio (per box) or the largest values (pooled)."""
    spec = MeasureSpec(hop=hop, band=list(bands_hz), energy_fraction=p)
    kbins = spec.bins(SR)
    rec, s0, s1, cls = (np.array([b[i] for b in boxes], dtype=np.int64) for i in range(4))
    ws = _ws(arrays)
    h = _host(measurements.measure_boxes(ws, rec, s0, s1, spec, class_id=cls, noise_power=noise))
    noise_h = noise.cpu().numpy() if noise is not None else None
    worst, pooled = [(0.0, 1.0), (0.0, 1.0)], [(0.0, 0.0), (0.0, 0.0)]
    assert h["frame_offsets"].tolist() == np.concatenate([[0], np.cumsum(h["n_frames"])]).tolist() and h["envelope"].shape == (h["frame_offsets"][-1],)
    assert h["spectrum"].shape == (len(boxes), 257) and h["spectrum"].dtype == np.float32 and h["envelope"].dtype == np.float32
    for e, (r, a, b, c) in enumerate(boxes):
        x, (lo, hi) = arrays[r], (int(kbins[c][0]), int(kbins[c][1]))
        got = _event(h, e)
        f0, n = M.event_frames(a, b, hop, len(x))
        assert (got["first_frame"], got["n_frames"]) == (f0, n) and len(got["envelope"]) == n, (e, boxes[e])
        assert (_bits(got["spectrum"][:lo]) == 0).all() and (_bits(got["spectrum"][hi:]) == 0).all()       # +0 outside the band
        if stats and n:
            P64, P32 = _power(x, hop)
            ref_s, ref_e, bad = M.stats_of_power(P64, f0, n, lo, hi)
            cpu_s, cpu_e, _ = M.stats_of_power(P32, f0, n, lo, hi)
            assert got["nonfinite"] == bad == 0
            if P64[f0:f0 + n].sum(axis=1).min() > 0.0:
                dev, cpu = M.deviations(got["spectrum"], got["envelope"], ref_s, ref_e, P64, f0, n), M.deviations(cpu_s, cpu_e, ref_s, ref_e, P64, f0, n)
                for j in range(2):
                    if not per_box:
                        pooled[j] = (max(pooled[j][0], dev[j]), max(pooled[j][1], cpu[j]))
                        continue
                    assert dev[j] <= 8.0 * cpu[j], (boxes[e], ("spectrum", "envelope")[j], dev[j], cpu[j])
                    if cpu[j] > 0 and dev[j] * worst[j][1] >= worst[j][0] * cpu[j]:          # the pair with the largest ratio
                        worst[j] = (dev[j], cpu[j])
        want = M.measure(got["spectrum"], got["envelope"], int(got["nonfinite"]), f0, lo, hi, hop, SR, p, None if noise_h is None else noise_h[r])
        for k in M.INTS:
            assert got[k] == want[k], (boxes[e], k, got[k], want[k])
        for k in M.FLOATS:
            g, w = float(got[k]), float(want[k])
            assert (math.isnan(g) and math.isnan(w)) or g == w or abs(g - w) <= 1e-9 * abs(w), (boxes[e], k, g, w)
        assert got["box_begin_s"] == a / SR and got["box_end_s"] == b / SR
    for j in range(2):
        assert pooled[j][0] <= 8.0 * pooled[j][1], (("spectrum", "envelope")[j], pooled[j])
    return h, worst if per_box else pooled


# ------------------------------------------------------------------------------------------------------------- 1. yardsticks that exist
@pytest.mark.parametrize("hop", A.HOPS)
def test_statistics_are_those_of_the_soundscape_kernels(built_lib, synth, hop):
    ws = _ws([synth])
    F = A.n_frames_of(len(synth), hop)
    one = soundscape.spectral_stats(ws, IndexSpec(hop=hop, segment_s=hop / SR))
    seg = soundscape.spectral_stats(ws, IndexSpec(hop=hop, segment_s=150 * hop / SR))
    assert one.segment_frames == 1 and seg.segment_frames == 150 and seg.n_frames.tolist()[:2] == [150, 150]
    frames = [0, 1, 63, 64, 200, F - 1]
    s0 = [f * hop for f in frames] + [150 * hop, 0, 3 * hop + 1]
    s1 = [f * hop + 512 for f in frames] + [299 * hop + 512, len(synth), 140 * hop + 511]
    m = measurements.measure_boxes(ws, [0] * len(s0), s0, s1, MeasureSpec(hop=hop))
    h = _host(m)
    assert h["n_frames"].tolist() == [1] * len(frames) + [150, F, 136] and h["first_frame"].tolist() == frames + [150, 0, 4]
    mean_power, frame_power = one.mean_power.cpu().numpy(), one.frame_power.cpu().numpy()
    for e, f in enumerate(frames):                                                          # a one-frame event: the frame's row
        assert np.array_equal(_bits(h["spectrum"][e]), _bits(mean_power[f])), f
    e = len(frames)                                                                         # runs of 64, 64 and 22 frames: segment 1 of S = 150
    assert np.array_equal(_bits(h["spectrum"][e] / np.float32(150)), _bits(seg.mean_power[1]))
    for e in range(len(s0)):                                                                # the full band: the frame's total power
        got = _event(h, e)
        assert np.array_equal(_bits(got["envelope"]), _bits(frame_power[got["first_frame"]:got["first_frame"] + got["n_frames"]])), e


# ------------------------------------------------------------------------------------------------------------- 2, 3. statistics and decisions
@pytest.mark.parametrize("hop", A.HOPS)
def test_statistics_and_decisions_against_float64(built_lib, synth, hop):
    """The boxes and bands of _measure_ref on the synthetic recording.  Measured on an MI355X -- device | float32 CPU chain, for spectrum
    and envelope: see DESIGN.md 4.11l.  The decisions from the samples: test_measurements_cpu.py asserts that every quantile has a margin
    of 1e-4 of the total on these inputs and that the float32 CPU chain agrees; peak_frame is compared through its envelope value (a steady
    tone is a near tie): |max envelope - max envelope64| <= max_t |envelope - envelope64| <= bar * max_t P_f."""
    boxes = [(0, a, b, c) for a, b in M.BOXES for c in range(3)]
    h, worst = _check([synth], boxes, hop)
    print(f"hop {hop}: spectrum device {worst[0][0]:.3e} | float32 CPU {worst[0][1]:.3e} (ratio {worst[0][0] / worst[0][1]:.2f}); "
          f"envelope device {worst[1][0]:.3e} | float32 CPU {worst[1][1]:.3e} (ratio {worst[1][0] / worst[1][1]:.2f})")
    P64, P32 = _power(synth, hop)
    for e, (_, a, b, c) in enumerate(boxes):
        lo, hi = M.BANDS[c]
        want = M.measure_box(P64, a, b, lo, hi, hop, SR, len(synth))
        got = _event(h, e)
        for k in ("n_frames", "low_bin", "centre_bin", "high_bin", "peak_bin", "low_frame", "centre_frame", "high_frame"):
            assert got[k] == want[k], (boxes[e], k, got[k], want[k])
        f0, n = want["first_frame"], want["n_frames"]
        cpu_e = M.stats_of_power(P32, f0, n, lo, hi)[1]
        pf = P64[f0:f0 + n].sum(axis=1)
        bar = 8.0 * float(np.max(np.abs(cpu_e.astype(np.float64) - want["envelope"]) / pf))
        assert f0 <= got["peak_frame"] < f0 + n
        assert abs(float(got["envelope"][got["peak_frame"] - f0]) - float(want["envelope"].max())) <= bar * float(pf.max()), (boxes[e], got["peak_frame"], want["peak_frame"])


# ------------------------------------------------------------------------------------------------------------- 4. run and span edges
@pytest.mark.parametrize("hop", [200, 512])
def test_run_and_span_edges(built_lib, synth, hop):
    """Events of 0, 1, 4, 5, 64, 65 and 129 frames (a step of four frames and a run of 64 with and without a rest), boxes at the
    recording's first sample and ending at its last, recordings of 511 (no frame), 512 (one) and 40 001 samples in one call, a one-bin
    band and the band that is bin 256 alone."""
    arrays = [synth[1000:1511], synth[17000:17512], synth[15000:55001]]
    bands = BANDS_HZ + ((3000.0, 3001.0), (8000.0, 8001.0))
    assert MeasureSpec(band=list(bands)).bins(SR)[3:].tolist() == [[96, 97], [256, 257]]
    n_long = len(arrays[2])
    f0 = -(-1000 // hop)
    boxes = [(2, 1000, 1400, 0)]                                                            # no frame
    for j, n in enumerate((1, 4, 5, 64, 65, 129)):
        if f0 * hop + (n - 1) * hop + 512 <= n_long:
            boxes.append((2, 1000, min(f0 * hop + (n - 1) * hop + 512 + 7, n_long), j % 5))
    boxes += [(2, 0, 512 + 4 * hop, 3), (2, 0, 700, 4), (2, n_long - 512 - 5 * hop, n_long, 4), (2, n_long - 512, n_long, 3), (2, 0, n_long, 1),
              (0, 0, 511, 0), (1, 0, 512, 2), (1, 0, 512, 4), (1, 1, 512, 0), (2, 20000, 20000, 0)]
    h, pooled = _check(arrays, boxes, hop, bands_hz=bands, per_box=False)
    print(f"hop {hop}, edges: spectrum device {pooled[0][0]:.3e} | float32 CPU {pooled[0][1]:.3e}; envelope device {pooled[1][0]:.3e} | float32 CPU {pooled[1][1]:.3e}")
    want_n = [M.event_frames(a, b, hop, len(arrays[r]))[1] for r, a, b, _ in boxes]
    assert h["n_frames"].tolist() == want_n and want_n[:2] == [0, 1] and want_n[-5:] == [0, 1, 1, 0, 0]
    if hop == 200:
        assert want_n[1:7] == [1, 4, 5, 64, 65, 129]
    empty = h["n_frames"] == 0
    assert (h["low_bin"][empty] == -1).all() and (h["peak_frame"][empty] == -1).all() and np.isnan(h["energy"][empty]).all() and (_bits(h["spectrum"][empty]) == 0).all()
    one_bin = [e for e, b in enumerate(boxes) if b[3] >= 3 and h["n_frames"][e] > 0]
    for e in one_bin:
        k = 96 if boxes[e][3] == 3 else 256
        assert h["low_bin"][e] == h["centre_bin"][e] == h["high_bin"][e] == h["peak_bin"][e] == k and h["bandwidth_hz"][e] == SR / 512
        assert float(h["energy"][e]) == float(h["spectrum"][e, k]) > 0


# ------------------------------------------------------------------------------------------------------------- 5. company
def test_bits_depend_on_the_event_alone(built_lib, synth):
    x, loud = synth[15000:55001], np.random.default_rng(5).choice([-1.0, 1.0], 30000).astype(np.float32)
    spec = MeasureSpec(hop=200, band=list(BANDS_HZ))
    boxes = [(1000, 14000, 0), (5000, 5512, 1), (0, 40001, 2), (12000, 30000, 1), (13000, 13300, 0), (26001, 39999, 2)]      # they overlap

    def run(arrays, r, order):
        rows = [boxes[i] for i in order]
        m = measurements.measure_boxes(_ws(arrays), [r] * len(rows), [b[0] for b in rows], [b[1] for b in rows], spec, class_id=[b[2] for b in rows])
        h = _host(m)
        return {i: _event(h, e) for e, i in enumerate(order)}, h

    alone = {i: run([x], 0, [i])[0][i] for i in range(len(boxes))}
    assert alone[0]["n_frames"] == 63 and alone[4]["n_frames"] == 0 and alone[2]["low_bin"] >= 32
    for arrays, r, order in (([x], 0, [0, 1, 2, 3, 4, 5]), ([x], 0, [5, 3, 1, 4, 2, 0]), ([x], 0, [2, 2, 0, 2, 5, 5]), ([x, loud], 0, [3, 0, 5, 1, 2, 4]),
                             ([loud, synth[:511], x], 2, [1, 2, 3]), ([x], 0, [0, 1, 2, 3, 4, 5])):
        got, h = run(arrays, r, order)
        assert (h["recording"] == r).all()
        for i in set(order):
            _same_bits(alone[i], got[i], (len(arrays), order, i))


# ------------------------------------------------------------------------------------------------------------- 6. poison and silence
def test_nan_and_inf_poison_their_events_only(built_lib, synth):
    hop = 200
    x = synth[:20000].copy()
    x[6000], x[15003] = np.nan, -np.inf
    boxes = [(0, 2000, 12000, 0), (0, 0, 5999, 1), (0, 6001, 15003, 2), (0, 5000, 16000, 0), (1, 2000, 12000, 0), (0, 15004, 20000, 1)]
    spec = MeasureSpec(hop=hop, band=list(BANDS_HZ))
    cols = [[b[i] for b in boxes] for i in range(4)]
    bad = _host(measurements.measure_boxes(_ws([x, synth[:20000]]), cols[0], cols[1], cols[2], spec, class_id=cols[3]))
    clean = _host(measurements.measure_boxes(_ws([synth[:20000], synth[:20000]]), cols[0], cols[1], cols[2], spec, class_id=cols[3]))
    want_bad = []
    for r, a, b, _ in boxes:
        f0, n = M.event_frames(a, b, hop, 20000)
        want_bad.append(sum(any(f * hop <= i < f * hop + 512 for i in (6000, 15003)) for f in range(f0, f0 + n)) if r == 0 else 0)
    assert want_bad == [3, 0, 0, 6, 0, 0] and bad["nonfinite"].tolist() == want_bad and clean["nonfinite"].tolist() == [0] * 6
    kbins = spec.bins(SR)
    for e, (r, a, b, c) in enumerate(boxes):
        got, ref = _event(bad, e), _event(clean, e)
        if want_bad[e] == 0:
            _same_bits(got, ref, e)                                                        # an event that avoids the sample: the bits of a clean run
            continue
        lo, hi = kbins[c]
        assert np.isnan(got["spectrum"][lo:hi]).all() and (_bits(got["spectrum"][:lo]) == 0).all() and (_bits(got["spectrum"][hi:]) == 0).all()
        assert all(got[k] == -1 for k in M.INTS[2:]) and all(math.isnan(got[k]) for k in M.FLOATS) and got["n_frames"] == ref["n_frames"]
        nan = np.isnan(got["envelope"])
        assert nan.sum() == want_bad[e] and np.array_equal(_bits(got["envelope"][~nan]), _bits(ref["envelope"][~nan]))      # the envelope keeps the per-frame values


def test_silence_beside_full_scale_is_plus_zero(built_lib):
    rng = np.random.default_rng(6)
    x = np.zeros(8192, dtype=np.float32)
    x[4096:] = rng.choice([-1.0, 1.0], 4096)
    x[700:900] = -0.0
    m = _host(measurements.measure_boxes(_ws([x]), [0, 0, 0], [0, 0, 100], [4096, 8192, 3000], MeasureSpec(hop=256)))
    for e in (0, 2):
        got = _event(m, e)
        assert got["n_frames"] > 0 and (_bits(got["spectrum"]) == 0).all() and (_bits(got["envelope"]) == 0).all() and got["nonfinite"] == 0      # +0, not -0
        assert got["energy"] == 0.0 and all(got[k] == -1 for k in M.INTS[2:]) and all(math.isnan(got[k]) for k in M.FLOATS[1:])
    mixed = _event(m, 1)
    assert mixed["low_frame"] >= 15 and mixed["energy"] > 0 and (_bits(mixed["envelope"][:15]) == 0).all()       # frames 0..14 lie wholly inside the zeros


# ------------------------------------------------------------------------------------------------------------- 7. noise
@pytest.mark.parametrize("hop", A.HOPS)
def test_noise_subtraction(built_lib, synth, hop):
    ws = _ws([synth, synth[:3000]])
    st = soundscape.spectral_stats(ws, IndexSpec(hop=hop, segment_s=16 * hop / SR))
    assert st.segment_frames == 16
    noise = measurements.noise_spectrum(st)
    want = M.noise_spectrum(st.mean_power.cpu().numpy(), st.n_frames, st.nonfinite_frames.cpu().numpy(), st.recording, 16, 2)
    assert noise.shape == (2, 257) and noise.dtype == torch.float32 and np.array_equal(_bits(noise), _bits(want))
    assert np.isfinite(want[0]).all() and np.isnan(want[1]).all()                            # 3000 samples hold no full segment
    h, _ = _check([synth, synth[:3000]], [(0, 0, 96123, 0), (0, 16000, 25600, 2), (0, 40000, 60000, 1)], hop, noise=noise, stats=False)
    assert (h["low_bin"][0], h["high_bin"][0]) == (95, 209) and np.isfinite(h["snr_db"]).all() and (h["snr_db"] > 0).all()
    plain = _host(measurements.measure_boxes(ws, [0], [0], [96123], MeasureSpec(hop=hop)))
    assert 0 < h["energy"][0] < plain["energy"][0] and np.array_equal(_bits(h["spectrum"][0]), _bits(plain["spectrum"][0]))
    # the event's own mean spectrum as the noise: nothing is left (64 frames: the division and the product are exact)
    box = ([0], [40 * hop], [40 * hop + 63 * hop + 512])
    own = measurements.measure_boxes(ws, *box, MeasureSpec(hop=hop))
    assert int(own["n_frames"][0]) == 64
    mean = torch.stack([own["spectrum"][0] / 64.0, torch.zeros(257, device="cuda")])
    left = _host(measurements.measure_boxes(ws, *box, MeasureSpec(hop=hop), noise_power=mean))
    assert _bits(left["energy"])[0] == 0 and left["snr_db"][0] == -math.inf and left["low_bin"][0] == -1 and left["peak_bin"][0] == -1
    assert left["low_frame"][0] >= 0                                                        # the envelope is not flat: some frames stand above their mean


# ------------------------------------------------------------------------------------------------------------- 8. entry points
class _RmsModel(ModelBase):
    """An embedding of one number: the window's RMS in dB over its valid samples."""

    def __init__(self):
        super().__init__("cuda", None)

    def register_hooks_for_layers(self, layers):
        self._hook_layers = ["rms"]
        return self._hook_layers

    def ensure_hooks_registered(self):
        pass

    def extract_embeddings(self, x, *, aggregation="mean", **kw):
        wav, pad = x["raw_wav"], x["padding_mask"]
        valid = (~pad).sum(1).clamp(min=1).to(torch.float32)
        return (10.0 * torch.log10((wav * wav).sum(1) / valid)).unsqueeze(1)


def test_events_padded_rows_and_detect_events(built_lib, synth):
    probe = torch.nn.Linear(1, 2).cuda()
    with torch.no_grad():
        probe.weight.copy_(torch.tensor([[0.1], [-0.1]]))
        probe.bias.copy_(torch.tensor([2.5, -2.5]))                                        # class 0: louder than -25 dB RMS; class 1: quieter
    spec = MeasureSpec(hop=200, band=[(2000.0, 8000.0), (0.0, 8001.0)])
    res = detection.detect_events(_RmsModel(), probe, [synth, synth[:30000]], 0.5, 0.25, on=0.0, measure=spec)
    count = int(res["count"])
    assert count >= 5 and "measurements" in res and set(res["class_id"].cpu().tolist()) == {0, 1}
    assert "measurements" not in detection.detect_events(_RmsModel(), probe, [synth[:30000]], 0.5, 0.25, on=0.0)
    ws = recordings.RecordingWindows([torch.from_numpy(synth).cuda(), torch.from_numpy(synth[:30000].copy()).cuda()], SR, 8000, 4000)
    events = {k: res[k] for k in ("sequence", "class_id", "first", "last")}
    again = measurements.measure_events(events, ws, spec)
    assert set(again) == set(res["measurements"])
    for k in again:
        assert np.array_equal(_bits(again[k]), _bits(res["measurements"][k])), k
    h = _host(again)
    first, last = res["first"].cpu().numpy(), res["last"].cpu().numpy()
    assert np.array_equal(h["box_begin_s"], ws.start_s[first]) and np.array_equal(h["box_end_s"], ws.end_s[last])
    loud = (res["class_id"].cpu().numpy() == 0) & (res["recording"].cpu().numpy() == 0)
    assert loud.sum() >= 2 and set(h["peak_bin"][loud].tolist()) <= {96, 208}               # the 3 kHz and 6.5 kHz bursts
    assert (h["begin_s"][loud] >= h["box_begin_s"][loud]).all() and (h["end_s"][loud] <= h["box_end_s"][loud]).all()
    # padded rows: max_events larger than count
    scores = torch.cat([probe(torch.full((3, 1), -10.0, device="cuda")), probe(torch.full((ws.n_windows - 3, 1), -40.0, device="cuda"))]).detach()
    padded = detection.decode_events(scores, windows=ws, on=0.0, max_events=6)
    exact = detection.decode_events(scores, windows=ws, on=0.0)
    n = int(exact["count"])
    assert 1 <= n < 6 and int(padded["count"]) == n
    mp, me = _host(measurements.measure_events(padded, ws, spec)), _host(measurements.measure_events(exact, ws, spec))
    assert mp["frame_offsets"].shape == (7,) and (mp["frame_offsets"][n:] == mp["frame_offsets"][n]).all()
    for k in me:
        if k == "frame_offsets":
            assert np.array_equal(mp[k][:n + 1], me[k])
        elif k == "envelope":
            assert np.array_equal(_bits(mp[k]), _bits(me[k]))
        else:
            assert np.array_equal(_bits(mp[k][:n]), _bits(me[k])), k
    for k in M.INTS + ("recording",):
        assert (mp[k][n:] == -1).all(), k
    for k in M.FLOATS + ("box_begin_s", "box_end_s"):
        assert np.isnan(mp[k][n:]).all(), k
    assert (_bits(mp["spectrum"][n:]) == 0).all()
    none = measurements.measure_events(detection.decode_events(scores, windows=ws, on=100.0), ws, spec)       # E = 0: nothing is launched
    assert none["spectrum"].shape == (0, 257) and none["envelope"].shape == (0,) and none["frame_offsets"].cpu().tolist() == [0] and none["low_bin"].shape == (0,)
    only_padded = measurements.measure_events(detection.decode_events(scores, windows=ws, on=100.0, max_events=2), ws, spec)
    assert only_padded["n_frames"].cpu().tolist() == [-1, -1] and only_padded["envelope"].shape == (0,)


def test_refusals_launch_nothing(built_lib, synth):
    ws = _ws([synth[:20000], synth[:511]])
    spec = MeasureSpec(hop=256)
    for args, kw in ((([2], [0], [512]), {}), (([0], [-1], [512]), {}), (([0], [600], [512]), {}), (([0], [0], [20001]), {}), (([1], [0], [512]), {}),
                     (([0, 0], [0], [512]), {}), (([0], [0], [512]), dict(noise_power=torch.zeros(3, 257, device="cuda"))),
                     (([0], [0], [512]), dict(noise_power=np.zeros((2, 257), np.float32))), (([0.5], [0], [512]), {})):
        with pytest.raises(ValueError):
            measurements.measure_boxes(ws, *args, spec, **kw)
    with pytest.raises(ValueError):
        measurements.measure_boxes(ws, [0], [0], [512], MeasureSpec(band=[(0, 4000), (4000, 8000)]))                      # no class_id
    with pytest.raises(ValueError):
        measurements.measure_boxes(ws, [0], [0], [512], MeasureSpec(band=[(0, 4000), (4000, 8000)]), class_id=[2])
    with pytest.raises(ValueError):
        measurements.measure_boxes(ws, [0], [0], [512], MeasureSpec(band=(9000, 10000)))
    with pytest.raises(TypeError):
        measurements.measure_boxes(ws, [0], [0], [512], {"hop": 256})
    m = measurements.measure_boxes(ws, [0, 0], [0, 3000], [9000, 20000], spec)
    torch.cuda.synchronize()
    pinned, table_dev, partials = m._keep[:3]
    table = pinned.numpy().view(measurements.EVENT_DTYPE).copy()
    before = [t.clone() for t in list(m.values()) + [partials]]
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    F, runs, pb = int(table["n_frames"].sum()), int(((table["n_frames"] + 63) // 64).sum()), partials.numel() * 4
    tab = soundscape.activity._tables_on(ws.wav.device)
    res = np.zeros(1, dtype=measurements.RESULT_DTYPE)
    for name in res.dtype.names:
        res[name][0] = m[name].data_ptr()

    def frames(wav_ptr=ws.wav.data_ptr(), n=ws.wav.numel(), host=table, hop=256, frames_=F, runs_=runs, part=partials.data_ptr(), bytes_=pb):
        return L.avexhip_measure_frames(wav_ptr, n, host.ctypes.data, table_dev.data_ptr(), 2, hop, tab.data_ptr(), frames_, runs_, part, bytes_, m["envelope"].data_ptr(), stream)

    def reduce(host=table, hop=256, q=(0.05, 0.5, 0.95), bytes_=pb, noise=None, n_rec=2, out=res):
        return L.avexhip_measure_reduce(host.ctypes.data, table_dev.data_ptr(), 2, hop, F, runs, partials.data_ptr(), bytes_, m["envelope"].data_ptr(), noise, n_rec, *q,
                                        m["spectrum"].data_ptr(), out.ctypes.data, stream)

    def changed(field, value, e=1):
        t = table.copy()
        t[field][e] = value
        return t

    for kw in (dict(wav_ptr=None), dict(wav_ptr=ws.wav.data_ptr() + 4), dict(hop=31), dict(hop=200), dict(frames_=F - 1), dict(runs_=runs + 1), dict(n=10000), dict(part=None),
               dict(host=changed("s1", 20001)), dict(host=changed("s0", 9001, 0)), dict(host=changed("hi", 258)), dict(host=changed("n_frames", 1)),
               dict(host=changed("base", ws.wav.numel()))):
        assert frames(**kw) == -1 and _capi.last_error().startswith("measure_frames"), kw
    assert frames(bytes_=pb - 4) == -4
    no_energy = res.copy()
    no_energy["energy"][0] = 0
    for kw in (dict(hop=513), dict(q=(0.5, 0.5, 1.0)), dict(q=(0.95, 0.5, 0.05)), dict(host=changed("lo", 257)), dict(host=changed("first_run", 0)),
               dict(noise=m["spectrum"].data_ptr(), n_rec=0), dict(out=no_energy)):
        assert reduce(**kw) == -1 and _capi.last_error().startswith("measure_reduce"), kw
    assert reduce(bytes_=pb - 4) == -4
    torch.cuda.synchronize()
    for a, b in zip(before, list(m.values()) + [partials]):
        assert np.array_equal(_bits(a), _bits(b))
