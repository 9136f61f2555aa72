"""Acoustic indices on the device: avex_amd.soundscape over csrc/soundscape.hip (avexhip_soundscape_frames / _reduce / _indices) against
tests/_soundscape_ref.py.

The fp32 statistics are compared with a float64 chain under bars measured in the same test: 8 x the same deviation of a float32 CPU chain
(torch.fft.rfft of the fp32 product, fp32 |.|^2, sqrt and sums), the project's standing margin for an fp32 transform against a float32 CPU
transform.  The indices, fp64 on the device, are compared with the restatement fed the device's own statistics, to 1e-9.  What must be
exact -- silence, counts at the two infinite thresholds, independence of a frame from its neighbours and of a recording from its company --
is compared bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import _activity_ref as A
import _soundscape_ref as S
from avex_amd import _capi, recordings, soundscape
from avex_amd.soundscape import IndexSpec

pytestmark = pytest.mark.gpu

SR = A.SR
FLOATS = ("mean_power", "mean_amplitude", "abs_diff")


def _ws(arrays):
    return recordings.RecordingWindows([torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in arrays], SR, 16000, 16000)


def _spec(hop, seg, **kw):
    spec = IndexSpec(hop=hop, segment_s=seg * hop / SR, **kw)
    assert spec.segment_frames(SR) == seg
    return spec


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _of(st, r):
    """Recording r of a SpectralStats, on the host, in the layout of _soundscape_ref.stats_of_power."""
    g0, g1 = st.segment_ranges[r]
    f0, f1 = st.frame_ranges[r]
    out = {k: getattr(st, k)[g0:g1].cpu().numpy() for k in FLOATS + ("count_above", "nonfinite_frames")}
    out["frame_power"] = st.frame_power[f0:f1].cpu().numpy()
    out["n_frames"] = st.n_frames[g0:g1]
    out["first_frame"] = np.cumsum(out["n_frames"]) - out["n_frames"]
    return out


@pytest.fixture(scope="module")
def synth():
    return A.synthetic()


@pytest.fixture(scope="module")
def power(synth):
    """The float64 reference and the float32 CPU chain of the synthetic recording, once per hop."""
    return {hop: (A.frame_power64(synth, hop), S.power32(synth, hop)) for hop in A.HOPS}


def _frame_power_deviation(fp, P64):
    return float(np.max(np.abs(fp.astype(np.float64) - P64.sum(axis=1)) / P64.sum(axis=1))) if len(P64) else 0.0


def _check_stats(arrays, hop, seg, db=-50.0, powers=None):
    """The statistics of every recording against float64 under the 8 x float32-CPU-chain bars; returns the device and CPU figures
    (mean_power, mean_amplitude, abs_diff, frame_power), each the maximum over the recordings."""
    st = soundscape.spectral_stats(_ws(arrays), _spec(hop, seg, db_threshold=db))
    dev, cpu = [0.0] * 4, [0.0] * 4
    g = 0
    for r, x in enumerate(arrays):
        P64, P32 = powers[r] if powers is not None else (A.frame_power64(x, hop), S.power32(x, hop))
        ref, ref32, got = S.stats_of_power(P64, seg, db), S.stats_of_power(P32, seg, db), _of(st, r)
        assert st.segment_ranges[r] == (g, g + len(ref["n_frames"])) and got["n_frames"].tolist() == ref["n_frames"].tolist(), r
        assert got["frame_power"].shape == (len(P64),) and got["nonfinite_frames"].tolist() == ref["nonfinite_frames"].tolist()
        g += len(ref["n_frames"])
        for k in FLOATS:
            assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (r, k)
        assert (got["abs_diff"][ref["n_frames"] == 1] == 0).all()                          # no difference inside a one-frame segment
        d, c = S.deviations(got, ref) + [_frame_power_deviation(got["frame_power"], P64)], S.deviations(ref32, ref) + [_frame_power_deviation(ref32["frame_power"], P64)]
        dev, cpu = [max(a, b) for a, b in zip(dev, d)], [max(a, b) for a, b in zip(cpu, c)]
    assert st.n_segments == g and st.mean_power.shape == (g, 257)
    print(f"hop {hop} S {seg}: device " + " ".join(f"{v:.3e}" for v in dev) + " | float32 CPU " + " ".join(f"{v:.3e}" for v in cpu))
    for name, d, c in zip(FLOATS + ("frame_power",), dev, cpu):
        assert d <= 8.0 * c, (name, d, c)
    return dev, cpu


# ------------------------------------------------------------------------------------------------------------- 1. statistics against fp64
@pytest.mark.parametrize("hop", A.HOPS)
def test_statistics_of_the_synthetic_recording(built_lib, synth, power, hop):
    """374 frames at hop 256 (a last segment of 54), 479 at hop 200 (a last segment of 31, frame starts off the 16-byte grid).
    Measured on an MI355X -- device | float32 CPU chain, for mean_power, mean_amplitude, abs_diff, frame_power: see DESIGN.md 4.11k."""
    assert len(power[hop][0]) == {256: 374, 200: 479}[hop]
    _check_stats([synth], hop, 64, powers=[power[hop]])


# ------------------------------------------------------------------------------------------------------------- 2. run and segment boundaries
def test_run_boundaries_inside_a_segment(built_lib, synth, power):
    """S = 150: runs of 64, 64 and 22 frames; a boundary difference dropped or counted twice shows at 1e-2 on abs_diff."""
    _check_stats([synth], 256, 150, powers=[power[256]])
    _check_stats([synth], 200, 1000, powers=[power[200]])                                  # one S larger than F: 479 frames, eight runs


@pytest.mark.parametrize("seg", [1, 2, 3, 7])
def test_short_segments(built_lib, synth, seg):
    _check_stats([synth[15000:55001]], 200, seg)


@pytest.mark.parametrize("hop", [200, 512])
def test_short_recordings_in_one_call(built_lib, synth, hop):
    """Recordings of 511 (no frame), 512 (one) and 40 001 samples; S = 70: runs of 64 and 6."""
    _check_stats([synth[1000:1511], synth[17000:17512], synth[15000:55001]], hop, 70)


# ------------------------------------------------------------------------------------------------------------- 3. a frame's bits are its own
def test_a_quiet_frame_does_not_see_its_neighbours(built_lib):
    rng = np.random.default_rng(3)
    q = [(1e-4 * rng.standard_normal(512)).astype(np.float32) for _ in range(4)]             # -80 dBFS
    l = [rng.choice([-1.0, 1.0], 512).astype(np.float32) for _ in range(4)]                  # full scale
    a, b = np.concatenate(q), np.concatenate([l[0], q[1], l[2], q[3]])
    st = soundscape.spectral_stats(_ws([a, b]), _spec(512, 1))
    assert st.segment_ranges == [(0, 4), (4, 8)]
    mp, fp = _bits(st.mean_power), _bits(st.frame_power)
    for g in (1, 3):
        assert np.array_equal(mp[g], mp[4 + g]) and fp[g] == fp[4 + g], g
    assert not np.array_equal(mp[0], mp[4]) and float(st.frame_power[4]) > 1e6 * float(st.frame_power[5])


# ------------------------------------------------------------------------------------------------------------- 4. bits depend on the recording alone
def test_bits_depend_on_the_recording_alone(built_lib, synth):
    x, short, other = synth[15000:55001], synth[:511], synth[60000:60700]
    spec = _spec(200, 70)

    def bits_of(arrays, r):
        ind = soundscape.acoustic_indices(_ws(arrays), spec)
        st = ind.stats
        g0, g1 = st.segment_ranges[r]
        f0, f1 = st.frame_ranges[r]
        return [_bits(getattr(st, k)[g0:g1]) for k in FLOATS + ("count_above", "nonfinite_frames")] + [_bits(st.frame_power[f0:f1]), _bits(ind.values[g0:g1])]

    alone = bits_of([x], 0)
    assert alone[0].shape == (3, 257) and alone[-1].shape == (3, 8)
    for arrays, r in (([x], 0), ([x, short, other], 0), ([short, x, other], 1), ([other, short, x], 2)):
        for a, b in zip(alone, bits_of(arrays, r)):
            assert np.array_equal(a, b), (len(arrays), r)


# ------------------------------------------------------------------------------------------------------------- 5. silence and non-finite samples
def test_silence_beside_full_scale_is_plus_zero(built_lib):
    rng = np.random.default_rng(5)
    x = np.zeros(6 * 512, dtype=np.float32)
    x[0:512] = rng.choice([-1.0, 1.0], 512)
    x[700:900] = -0.0
    x[3 * 512:4 * 512] = rng.choice([-1.0, 1.0], 512)
    ind = soundscape.acoustic_indices(_ws([x]), _spec(512, 1))
    st = ind.stats
    silent = [1, 2, 4, 5]
    for k in FLOATS:
        assert (_bits(getattr(st, k))[silent] == 0).all(), k                                 # +0, not a rounding residue and not -0
    assert (_bits(st.frame_power)[silent] == 0).all() and (st.count_above.cpu().numpy()[silent] == 0).all()
    assert (st.mean_power.cpu().numpy()[[0, 3]] > 0).all() and st.nonfinite_frames.cpu().tolist() == [0] * 6
    v = ind.values.cpu().numpy()
    assert np.array_equal(np.isnan(v[silent]), np.broadcast_to([False, True, True, False, True, True, True, True], (4, 8)))
    assert (v[silent][:, [0, 3]] == 0).all()                                                 # aci = 0 and bi = 0 in silence


def test_nan_and_inf_poison_their_segments_only(built_lib, synth):
    """hop 200, S = 5: sample 1000 lies in frames 3..5 and sample 5003 in frames 23..25, each across a segment boundary (two segments).
    db_threshold = -inf: count_above is then the number of finite frames, in every bin."""
    hop, seg = 200, 5
    x = synth[:8000].copy()
    x[1000], x[5003] = np.nan, -np.inf
    spec = _spec(hop, seg, db_threshold=-math.inf)
    ind = soundscape.acoustic_indices(_ws([x, synth[:4000]]), spec)
    clean = soundscape.acoustic_indices(_ws([synth[:8000], synth[:4000]]), spec)
    ref = S.stats64(x, hop, seg, -math.inf)
    F, G = A.n_frames_of(8000, hop), len(ref["n_frames"])
    assert (F, G) == (38, 8) and ref["nonfinite_frames"].tolist() == [2, 1, 0, 0, 2, 1, 0, 0]
    st, cl = ind.stats, clean.stats
    bad = np.zeros(st.n_segments, dtype=bool)
    bad[:G] = ref["nonfinite_frames"] > 0
    assert st.nonfinite_frames.cpu().tolist()[:G] == ref["nonfinite_frames"].tolist() and not st.nonfinite_frames[G:].any().item()
    for k in FLOATS:
        got = getattr(st, k).cpu().numpy()
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all(), k
        assert np.array_equal(_bits(got[~bad]), _bits(getattr(cl, k))[~bad]), k               # the neighbours: the bits of a clean run
    counts = st.count_above.cpu().numpy()
    n = st.n_frames.astype(np.int64)
    assert np.array_equal(counts[:G], np.broadcast_to((n[:G] - ref["nonfinite_frames"])[:, None], (G, 257)))
    assert np.array_equal(counts[~bad], cl.count_above.cpu().numpy()[~bad])
    holds = np.array([any(f * hop <= i < f * hop + 512 for i in (1000, 5003)) for f in range(F)])
    fp, fp_clean = st.frame_power.cpu().numpy(), cl.frame_power.cpu().numpy()
    assert holds.sum() == 6 and np.isnan(fp[:F][holds]).all() and np.array_equal(_bits(fp[:F][~holds]), _bits(fp_clean[:F][~holds]))
    assert np.array_equal(_bits(fp[F:]), _bits(fp_clean[F:]))
    v, v_clean = ind.values.cpu().numpy(), clean.values.cpu().numpy()
    assert np.isnan(v[bad]).all() and np.array_equal(_bits(v[~bad]), _bits(v_clean[~bad])) and not np.isnan(v[~bad][:, 0]).any()


# ------------------------------------------------------------------------------------------------------------- 6. counts, exact
def test_counts_at_the_infinite_thresholds(built_lib):
    rng = np.random.default_rng(6)
    x = np.zeros(8 * 512, dtype=np.float32)
    loud = [0, 2, 3, 6]                                                                       # frames of noise; the others are zeros
    for f in loud:
        x[f * 512:(f + 1) * 512] = 0.05 * rng.standard_normal(512)
    want = np.array([sum(f in loud for f in range(g * 3, min(g * 3 + 3, 8))) for g in range(3)])
    st = soundscape.spectral_stats(_ws([x]), _spec(512, 3, db_threshold=-math.inf))
    assert st.n_frames.tolist() == [3, 3, 2] and want.tolist() == [2, 1, 1]
    assert np.array_equal(st.count_above.cpu().numpy(), np.broadcast_to(want[:, None], (3, 257)))
    st = soundscape.spectral_stats(_ws([x]), _spec(512, 3, db_threshold=math.inf))
    assert not st.count_above.any().item() and (st.mean_power.cpu().numpy() > 0).all()


# ------------------------------------------------------------------------------------------------------------- 7. counts against fp64
@pytest.mark.parametrize("hop", A.HOPS)
@pytest.mark.parametrize("which", ["synthetic at -50 dBFS", "noise at -60 dBFS"])
def test_counts_against_float64(built_lib, synth, power, hop, which):
    """Per (segment, bin) the count may differ from the float64 one by at most the cells with |P64 - thr| <= bar * P_f, bar = 8 x the
    per-cell deviation of the float32 CPU chain; those allowances are at most 0.1 % of the input's cells (asserted first, and without a
    GPU in tests/test_soundscape_cpu.py).  -60 dBFS is used on the noise-only stretch alone: on the whole recording P_f during the bursts
    is 500 x the noise and 4 - 5 % of the cells would be allowed."""
    if which.startswith("synthetic"):
        x, db, (P64, P32) = synth, -50.0, power[hop]
    else:
        x, db = synth[27200:49600], -60.0
        P64, P32 = A.frame_power64(x, hop), S.power32(x, hop)
    allow, bar = S.count_allowance(P64, P32, 64, db)
    assert allow.sum() <= 1e-3 * P64.size
    want = S.stats_of_power(P64, 64, db)["count_above"]
    got = soundscape.spectral_stats(_ws([x]), _spec(hop, 64, db_threshold=db)).count_above.cpu().numpy()
    diff = np.abs(got.astype(np.int64) - want)
    print(f"hop {hop}, {which}: bar {bar:.3e}, allowed {int(allow.sum())} of {P64.size} cells, differing {int(diff.sum())}; {want.sum() / P64.size:.3f} of the cells above")
    assert got.shape == want.shape and (diff <= allow).all()


# ------------------------------------------------------------------------------------------------------------- 8. indices from the statistics
def _check_indices(arrays, spec):
    """Every column equals the restatement fed the device's own statistics, to 1e-9 * max(1, |want|), NaN where NaN.  fp64 sums of at most
    a few thousand terms and logarithms good to a few ulp give under 1e-12; 1e-9 leaves room and is three orders under the statistics'
    own fp32 error."""
    ind = soundscape.acoustic_indices(_ws(arrays), spec)
    st, values = ind.stats, ind.values.cpu().numpy()
    assert values.shape == (st.n_segments, 8) and values.dtype == np.float64
    for r in range(len(arrays)):
        g0, _ = st.segment_ranges[r]
        got = _of(st, r)
        want = S.indices_of(got, spec, SR)
        have = values[g0:g0 + len(want)]
        assert np.array_equal(np.isnan(have), np.isnan(want)), (r, have, want)
        ok = np.isnan(want) | (np.abs(have - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))
        assert ok.all(), (r, have, want)
    for c, name in enumerate(soundscape.INDEX_NAMES):
        assert np.array_equal(_bits(ind.column(name)), _bits(values[:, c]))
    return ind, values


def test_indices_follow_from_the_statistics(built_lib, synth):
    silent = np.zeros(2000, dtype=np.float32)
    _, v = _check_indices([synth, silent], _spec(256, 64))                                   # the defaults: J = 8, clipped at Nyquist
    assert np.isfinite(v[:6, [0, 3, 4, 5, 6, 7]]).all()
    assert np.array_equal(np.isnan(v[6]), [False, True, True, False, True, True, True, True]) and v[6, 0] == 0 and v[6, 3] == 0      # the silent segment
    other = dict(band=(500.0, 7000.0), bio_band=(3000.0, 7000.0), anthro_band=(0.0, 1500.0), adi_step_hz=500.0, db_threshold=-65.0)
    _, v = _check_indices([synth, silent], _spec(200, 150, **other))                         # J = 16, every band occupied
    assert np.isfinite(v[:4]).all()
    _, v = _check_indices([synth], _spec(256, 64, adi_step_hz=8000.0, adi_max_hz=8000.0, db_threshold=-60.0))       # J = 1: adi = 0, aei = 0
    assert (v[:, 1] == 0).all() and (v[:, 2] == 0).all()
    ind, v = _check_indices([synth], _spec(256, 373))                                        # 374 frames: a last segment of one frame
    assert ind.n_frames.tolist() == [373, 1] and math.isnan(v[1, 6]) and math.isnan(v[1, 7]) and v[1, 0] == 0 and np.isfinite(v[1, 5])
    t = ind.table()
    assert list(t) == ["recording", "start_s", "end_s", "n_frames"] + list(soundscape.INDEX_NAMES)
    assert t["recording"].tolist() == [0, 0] and t["start_s"].tolist() == [0.0, 373 * 256 / SR] and t["end_s"].tolist() == [(372 * 256 + 512) / SR, (373 * 256 + 512) / SR]
    assert np.array_equal(_bits(t["hf"]), _bits(v[:, 5]))


# ------------------------------------------------------------------------------------------------------------- 9. end to end
BURSTS_3K = ((1.0, 1.6), (3.2, 3.25))
BURSTS = BURSTS_3K + ((4.5, 5.2),)


def _holding(ind, bursts):
    return np.array([any(s < t1 and e > t0 for t0, t1 in bursts) for s, e in zip(ind.start_s, ind.end_s)])


@pytest.mark.parametrize("hop", A.HOPS)
def test_indices_of_the_synthetic_recording(built_lib, synth, power, hop):
    """Each column against the float64 chain: the maximum over the segments of |index - index64| is at most 8 x the same figure of the
    float32 CPU chain (figures in DESIGN.md 4.11k), plus the 1e-9 * max(1, |index64|) that test_indices_follow_from_the_statistics allows the
    fp64 evaluation itself: adi and aei are functions of integer counts, the float32 CPU chain's counts equal the float64 ones on this
    input, so its deviation is exactly 0 and the bare 8 x rule would ask for the restatement's last fp64 bit (the device is 2.2e-16 off).
    Then three readings, each asserted on the reference's values and on the device's:

    * ndsi: every segment that holds a 3 kHz burst lies ABOVE every noise-only segment (burst power lands in bio_band, b >> a).  The
      6.5 kHz burst lies in bio_band as well, so its segments are as high; "the largest" holds against the noise-only ones.
    * hf: every burst segment lies BELOW every noise-only segment (one line against a flat spectrum).
    * adi at -50 dBFS: NaN where the reference is NaN and only there.  The noise sits near -59 dBFS per bin ON AVERAGE, but a Gaussian
      noise bin is exponentially distributed: about exp(-8), 3e-4, of its cells stand 9 dB over their mean, a handful per segment, so the
      reference's adi there is a number (small: few bands occupied), not NaN.  At -40 dBFS (19 dB over) no noise cell counts and adi IS
      NaN in the noise-only segments, in the reference and on the device."""
    P64, P32 = power[hop]
    spec = _spec(hop, 64)
    ind = soundscape.acoustic_indices(_ws([synth]), spec)
    got = ind.values.cpu().numpy()
    want, cpu = S.indices_of(S.stats_of_power(P64, 64, -50.0), spec, SR), S.indices_of(S.stats_of_power(P32, 64, -50.0), spec, SR)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(cpu), np.isnan(want))
    for c, name in enumerate(soundscape.INDEX_NAMES):
        d, bar = np.nanmax(np.abs(got[:, c] - want[:, c])), np.nanmax(np.abs(cpu[:, c] - want[:, c]))
        print(f"hop {hop} {name}: device {d:.3e}, float32 CPU {bar:.3e}")
    for c, name in enumerate(soundscape.INDEX_NAMES):
        bar = 8.0 * np.nanmax(np.abs(cpu[:, c] - want[:, c])) + 1e-9 * max(1.0, np.nanmax(np.abs(want[:, c])))
        assert np.nanmax(np.abs(got[:, c] - want[:, c])) <= bar, name

    tone3, tone, noise = _holding(ind, BURSTS_3K), _holding(ind, BURSTS), ~_holding(ind, BURSTS)
    assert tone3.sum() >= 2 and noise.sum() >= 1 and tone.sum() > tone3.sum()
    quiet = soundscape.acoustic_indices(_ws([synth]), _spec(hop, 64, db_threshold=-40.0)).values.cpu().numpy()
    want_quiet = S.indices_of(S.stats_of_power(P64, 64, -40.0), spec, SR)
    for v, q in ((want, want_quiet), (got, quiet)):
        assert v[tone3, 4].min() > v[noise, 4].max()
        assert v[tone, 5].max() < v[noise, 5].min()
        assert np.isnan(q[noise, 1]).all() and not np.isnan(q[tone3, 1]).any()
    assert not np.isnan(want[noise, 1]).any()


# ------------------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_launch_nothing(built_lib, synth):
    ws = _ws([synth[:20000], synth[:511]])
    st = soundscape.spectral_stats(ws, _spec(256, 30))
    ind = soundscape.SoundscapeIndices(st)
    torch.cuda.synchronize()
    before = [t.clone() for t in (st.mean_power, st.mean_amplitude, st.abs_diff, st.count_above, st.nonfinite_frames, st.frame_power, st._partials, ind.values)]
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    host, dev, n_rec = st._rec.ctypes.data, st._rec_dev.data_ptr(), 2
    wav, tab = ws.wav, soundscape.activity._tables_on(ws.wav.device)
    F, G, pb = st.total_frames, st.n_segments, st._partials_bytes
    moved = st._rec.copy()
    moved["base"][1] = wav.numel()                                                            # leaves the buffer

    def frames(wav_ptr=wav.data_ptr(), n=wav.numel(), table=host, hop=256, seg=30, thr=1.0, tables=tab.data_ptr(), frames_=F, part=st._partials.data_ptr(), bytes_=pb):
        return L.avexhip_soundscape_frames(wav_ptr, n, table, dev, n_rec, hop, seg, thr, tables, frames_, G, part, bytes_, st.frame_power.data_ptr(), stream)

    for kw in (dict(wav_ptr=None), dict(wav_ptr=wav.data_ptr() + 4), dict(tables=None), dict(hop=31), dict(hop=513), dict(seg=0), dict(seg=20), dict(thr=math.nan),
               dict(thr=-1.0), dict(frames_=F - 1), dict(table=moved.ctypes.data), dict(n=10000), dict(part=None)):
        assert frames(**kw) == -1 and _capi.last_error().startswith("soundscape_frames"), kw
    assert frames(bytes_=pb - 4) == -4
    tensors = (st.mean_power, st.mean_amplitude, st.abs_diff, st.count_above, st.nonfinite_frames)
    assert L.avexhip_soundscape_reduce(host, dev, n_rec, 256, 20, F, G, st._partials.data_ptr(), pb, *[t.data_ptr() for t in tensors], stream) == -1
    assert L.avexhip_soundscape_reduce(host, dev, n_rec, 256, 30, F, G, st._partials.data_ptr(), pb, None, *[t.data_ptr() for t in tensors[1:]], stream) == -1
    assert L.avexhip_soundscape_reduce(host, dev, n_rec, 256, 30, F, G, st._partials.data_ptr(), pb - 4, *[t.data_ptr() for t in tensors], stream) == -4
    good = ind._spec_bins
    for field, value in (("band", (0, 258)), ("bio", (9, 9)), ("anthro", (-1, 3)), ("n_adi", 0), ("n_adi", 33), ("bin_khz", math.nan)):
        sp = good.copy()
        sp[field][0] = value
        rc = L.avexhip_soundscape_indices(host, dev, n_rec, 256, 30, F, G, sp.ctypes.data, *[t.data_ptr() for t in tensors], st.frame_power.data_ptr(),
                                          ind.values.data_ptr(), stream)
        assert rc == -1 and _capi.last_error().startswith("soundscape_indices"), field
    with pytest.raises(ValueError):
        soundscape.acoustic_indices(ws, IndexSpec(bio_band=(9000, 10000)))
    with pytest.raises(TypeError):
        soundscape.acoustic_indices(ws, {"hop": 256})
    torch.cuda.synchronize()
    after = (st.mean_power, st.mean_amplitude, st.abs_diff, st.count_above, st.nonfinite_frames, st.frame_power, st._partials, ind.values)
    for a, b in zip(before, after):
        assert np.array_equal(_bits(a), _bits(b))


def test_the_convenience_call_and_no_segment_at_all(built_lib, synth):
    ind = soundscape.acoustic_indices_of([synth, synth[:300]], IndexSpec(segment_s=2.0))
    want = soundscape.acoustic_indices(_ws([synth, synth[:300]]), IndexSpec(segment_s=2.0))
    assert ind.segment_ranges == [(0, 3), (3, 3)] and np.array_equal(_bits(ind.values), _bits(want.values))
    assert ind.n_frames.tolist() == [125, 125, 124] and ind.table()["recording"].tolist() == [0, 0, 0]
    none = soundscape.acoustic_indices(_ws([synth[:300], synth[:511]]), IndexSpec())
    assert none.values.shape == (0, 8) and none.stats.mean_power.shape == (0, 257) and none.table()["aci"].shape == (0,)
