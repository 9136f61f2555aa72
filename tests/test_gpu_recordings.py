"""Whole-recording windows on the device: avex_amd.recordings over csrc/windows.hip (avexhip_window_stats / _select / _gather).

1. every row and mask is BIT-identical to the shipped per-file path (ingest.load_batch with the same starts), in one call or in chunks;
2. the statistics are exact where exactness is possible, within the fp64 summation bound otherwise, and depend on the window alone;
3. the gate's kept list and count equal the NumPy restatement (tests/_recordings_ref.py), across the scan's 1 024-window passes;
4. embed_recording / embed_recordings give the bits of one direct extract_embeddings call, whatever the batch size or the neighbours;
5. a recording over the resident limit and a table that leaves its recording are refused.
"""
import io
import wave

import numpy as np
import pytest
import torch

import _recordings_ref as R
import avex_amd
from avex_amd import _capi, ingest, recordings, synth

pytestmark = pytest.mark.gpu


def _wav16(x, sr):
    """[frames, channels] float in [-1, 1) -> 16-bit PCM WAV bytes."""
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(x.shape[1]); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((x * 32767).astype("<i2").tobytes())
    return buf.getvalue()


def _table(rows):
    """avexhip_window rows (base, n_samples, start, valid) -> (host table, the same bytes on the device)."""
    tab = np.zeros(len(rows), dtype=recordings.WINDOW_DTYPE)
    for i, (base, n, start, valid) in enumerate(rows):
        tab[i] = (base, n, start, valid, 0)
    return tab, torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).cuda()


def _stats(wav, rows, window_len):
    """avexhip_window_stats on a hand-made table: (energy, peak) as NumPy arrays."""
    tab, dev = _table(rows)
    e = torch.empty(len(rows), dtype=torch.float64, device="cuda")
    p = torch.empty(len(rows), dtype=torch.float32, device="cuda")
    _capi.check(_capi.lib().avexhip_window_stats(wav.data_ptr(), wav.numel(), tab.ctypes.data, dev.data_ptr(), len(rows), window_len, e.data_ptr(), p.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "window_stats")
    return e.cpu().numpy(), p.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------ 1. rows
_FILE = {}


def _file_441():
    if not _FILE:
        x = synth.normal("rec441", (50001, 3), 0.3).astype(np.float32).clip(-0.99, 0.99)
        _FILE["data"] = _wav16(x, 44100)
    return _FILE["data"]


@pytest.mark.parametrize("hop,n_windows,last_valid", [(1237, 15, 823), (907, 21, 1)])
def test_rows_are_bit_identical_to_load_batch(built_lib, hop, n_windows, last_valid):
    data, W = _file_441(), 4001
    ws = recordings.windows(data, W / 16000, hop / 16000, tail="pad")
    assert ws.wav.numel() == 18141 and ws.window_len == W and ws.hop_len == hop              # ceil(50001 * 16000 / 44100)
    n = ws.n_windows
    assert n == n_windows and int(ws.valids[-1]) == last_valid and ws.starts.tolist() == [hop * k for k in range(n)]
    assert np.array_equal(ws.start_s, ws.starts / 16000.0) and np.array_equal(ws.end_s, (ws.starts + ws.valids) / 16000.0) and ws.start_s.dtype == np.float64
    wav, mask = ws.batch(0, n)
    assert wav.shape == mask.shape == (n, W) and wav.dtype == torch.float32 and mask.dtype == torch.bool and wav.is_cuda and mask.is_cuda
    ref_wav, ref_mask, lengths = ingest.load_batch([data] * n, 16000, W, starts=ws.starts.tolist())
    assert lengths.tolist() == ws.valids.tolist()
    assert torch.equal(wav, ref_wav) and torch.equal(mask, ref_mask)
    r_wav, r_mask = R.rows(ws.wav.cpu().numpy(), ws.starts.tolist(), ws.valids.tolist(), W)     # and the restatement: slice, zeros, mask
    assert np.array_equal(wav.cpu().numpy(), r_wav) and np.array_equal(mask.cpu().numpy(), r_mask)
    for lo in range(0, n, 3):                                                                    # chunks of 3, the last one partial or single
        w3, m3 = ws.batch(lo, min(lo + 3, n))
        assert torch.equal(w3, wav[lo:lo + 3]) and torch.equal(m3, mask[lo:lo + 3]), lo
    order = torch.tensor([n - 1, 0, 5, 5, 2])
    for idx in (order, order.cuda(), order.numpy(), order.tolist()):                             # a list of window numbers, any order, repeats
        wi, mi = ws.batch(idx)
        assert torch.equal(wi, wav[order.cuda()]) and torch.equal(mi, mask[order.cuda()])
    wi, mi = ws.batch(torch.tensor([1, n, -1], device="cuda"))                                   # a device index is not copied back: outside -> empty row
    assert torch.equal(wi[0], wav[1]) and not wi[1:].any() and bool(mi[1:].all())
    with pytest.raises(IndexError):
        ws.batch(torch.tensor([0, n]))
    with pytest.raises(IndexError):
        ws.batch(3, n + 1)
    assert ws.batch(2, 2)[0].shape == (0, W)


def test_rows_tail_drop_short_recording_and_aligned_rows(built_lib):
    x = synth.normal("recrows", (5000,), 0.3).astype(np.float32)
    ws = recordings.windows(x, 1024 / 16000, 512 / 16000, tail="drop")                           # every start and the row length multiples of 4: the wide paths
    assert ws.n_windows == 8 and (ws.valids == 1024).all()
    wav, mask = ws.batch(0, 8)
    r_wav, r_mask = R.rows(x, ws.starts.tolist(), ws.valids.tolist(), 1024)
    assert np.array_equal(wav.cpu().numpy(), r_wav) and not mask.any()
    ws = recordings.windows(x, 1024 / 16000, 512 / 16000, tail="pad")                            # aligned rows whose valid part ends inside a group of four
    assert ws.n_windows == 10 and ws.valids[-2:].tolist() == [904, 392]
    wav, mask = ws.batch(0, 10)
    r_wav, r_mask = R.rows(x, ws.starts.tolist(), ws.valids.tolist(), 1024)
    assert np.array_equal(wav.cpu().numpy(), r_wav) and np.array_equal(mask.cpu().numpy(), r_mask)
    for tail in ("pad", "drop"):                                                                 # shorter than one window: one padded window under both
        ws = recordings.windows(x[:333], 0.25, tail=tail)
        assert ws.n_windows == 1 and ws.valids.tolist() == [333] and ws.hop_len == ws.window_len == 4000
        wav, mask = ws.batch(0, 1)
        assert np.array_equal(wav[0, :333].cpu().numpy(), x[:333]) and not wav[0, 333:].any() and mask[0].tolist() == [False] * 333 + [True] * 3667


# ------------------------------------------------------------------------------------------------------------------------ 2. statistics
W_ST, HOP_ST, N_ST = 4001, 1237, 20000           # three full 1 024-sample passes and a partial one; starts of every alignment mod 4


def test_statistics_are_exact_for_int16_samples(built_lib):
    m = np.random.default_rng(11).integers(-32768, 32768, size=N_ST).astype(np.int64)
    m[5000:9100] = 0                                                                             # a run of exact zeros inside windows 1 .. 7
    x = (m.astype(np.float32) * np.float32(2.0 ** -15))
    ws = recordings.windows(x, W_ST / 16000, HOP_ST / 16000)
    starts, valids = ws.starts.tolist(), ws.valids.tolist()
    assert ws.n_windows == 17 and valids[-1] == N_ST - 16 * HOP_ST == 208 and {s % 4 for s in starts} == {0, 1, 2, 3}
    want_e = np.array([int((m[s:s + v] ** 2).sum()) for s, v in zip(starts, valids)], dtype=np.int64)
    assert want_e.max() < 2 ** 53
    want_p = np.array([np.abs(m[s:s + v]).max() for s, v in zip(starts, valids)], dtype=np.int64)
    e, p = ws.energy.cpu().numpy(), ws.peak.cpu().numpy()
    assert e.dtype == np.float64 and p.dtype == np.float32
    assert (e == want_e.astype(np.float64) * 2.0 ** -30).all(), np.flatnonzero(e != want_e * 2.0 ** -30)
    assert (p == (want_p.astype(np.float64) * 2.0 ** -15).astype(np.float32)).all()
    r_rms, r_pk = R.db(*R.stats(x, starts, valids), valids)
    assert np.array_equal(ws.rms_db, r_rms) and np.array_equal(ws.peak_db, r_pk) and ws.rms_db.dtype == np.float64


def test_statistics_of_noise_silence_and_nan(built_lib):
    x = synth.normal("recstat", (N_ST,), 0.1).astype(np.float32)
    x[2 * HOP_ST:2 * HOP_ST + W_ST] = 0.0                                                        # window 2 is all zeros
    ws = recordings.windows(x, W_ST / 16000, HOP_ST / 16000)
    starts, valids = ws.starts.tolist(), ws.valids.tolist()
    e = ws.energy.cpu().numpy()
    for w, (s, v) in enumerate(zip(starts, valids)):
        ref = np.sum(x[s:s + v].astype(np.float64) ** 2)
        assert abs(e[w] - ref) <= 2 * v * 2.0 ** -53 * ref, (w, e[w], ref)                       # two fp64 sums of exact terms, each within v * 2^-53
    assert np.array_equal(ws.peak.cpu().numpy(), R.stats(x, starts, valids)[1])
    assert e[2] == 0.0 and ws.rms_db[2] == -np.inf and ws.peak_db[2] == -np.inf and np.isfinite(np.delete(ws.rms_db, 2)).all()
    bad = x.copy()
    bad[7 * HOP_ST + 5] = np.nan                                                                 # in windows 4 .. 7
    bad[15 * HOP_ST + 100] = np.inf                                                              # in windows 12 .. 15
    wb = recordings.windows(bad, W_ST / 16000, HOP_ST / 16000)
    eb = wb.energy.cpu().numpy()
    hit = [w for w, (s, v) in enumerate(zip(starts, valids)) if s <= 7 * HOP_ST + 5 < s + v or s <= 15 * HOP_ST + 100 < s + v]
    assert hit == [4, 5, 6, 7, 12, 13, 14, 15]
    assert np.isnan(eb[hit]).all() and np.isnan(wb.rms_db[hit]).all()
    rest = [w for w in range(len(starts)) if w not in hit]
    assert np.array_equal(eb[rest], e[rest])
    sel = wb.select().cpu().numpy()                                                              # both thresholds off: everything but the NaN windows
    assert sel[-1] == len(rest) and sel[:len(rest)].tolist() == rest == R.select(eb, wb.peak.cpu().numpy(), valids)


def test_statistics_depend_on_the_window_alone(built_lib):
    x = synth.normal("recstat", (N_ST,), 0.1).astype(np.float32)
    ws = recordings.windows(x, W_ST / 16000, HOP_ST / 16000)
    e, p = ws.energy.cpu().numpy(), ws.peak.cpu().numpy()
    starts, valids = ws.starts.tolist(), ws.valids.tolist()
    n = ws.n_windows
    for w in (0, 3, 9, n - 1):                                                                   # alone: a launch of one window
        e1, p1 = _stats(ws.wav, [(0, N_ST, starts[w], valids[w])], W_ST)
        assert e1[0] == e[w] and p1[0] == p[w], w
    rev = [(0, N_ST, starts[w], valids[w]) for w in reversed(range(n))]                          # another order, two chunks
    e2, p2 = _stats(ws.wav, rev[:5], W_ST)
    e3, p3 = _stats(ws.wav, rev[5:], W_ST)
    assert np.array_equal(np.concatenate([e2, e3])[::-1], e) and np.array_equal(np.concatenate([p2, p3])[::-1], p)
    for shift in (1, 2, 3):                                                                      # the same samples at another alignment: scalar instead of wide loads
        moved = torch.cat([torch.zeros(shift, device="cuda"), ws.wav])
        e4, _ = _stats(moved, [(shift, N_ST, s, v) for s, v in zip(starts, valids)], W_ST)
        assert np.array_equal(e4, e), shift
    other = torch.from_numpy(synth.normal("recother", (3001,), 0.2).astype(np.float32)).cuda()   # beside another recording, in one table
    both = recordings.RecordingWindows([other, ws.wav], 16000, W_ST, HOP_ST)
    w0, w1 = both.ranges[1]
    assert both.ranges[0] == (0, 3) and w1 - w0 == n and int(both._table["base"][w0]) == 3004
    assert torch.equal(both.energy[w0:w1], ws.energy) and torch.equal(both.peak[w0:w1], ws.peak)
    wav_a, mask_a = ws.batch(0, n)
    wav_b, mask_b = both.batch(w0, w1)
    assert torch.equal(wav_a, wav_b) and torch.equal(mask_a, mask_b)


# ------------------------------------------------------------------------------------------------------------------------ 3. selection
W_SEL, HOP_SEL, N_SEL, BLOCK = 64, 16, 20000, 1008       # 1 250 windows: the scan takes two passes; blocks are a multiple of the hop
SPIKES = (0, 1500, 3030, 9999, 16400, 19000)            # full-scale samples, in zero blocks and in noise blocks


def _alternating():
    x = synth.normal("recsel", (N_SEL,), 0.1).astype(np.float32).clip(-0.25, 0.25)
    for b in range(0, N_SEL, 2 * BLOCK):
        x[b:b + BLOCK] = 0.0                              # exact zeros alternate with noise of amplitude 0.1
    x[list(SPIKES)] = 1.0
    return x


def _check_gate(ws, x, min_rms_db, min_peak_db, margin_db=6.0):
    """select() against the restatement; every finite statistic sits at least margin_db from the threshold it is compared with."""
    valids = ws.valids.tolist()
    e, p = R.stats(x, ws.starts.tolist(), valids)
    rms, pk = R.db(e, p, valids)
    if min_rms_db is not None:
        assert np.abs(rms[np.isfinite(rms)] - min_rms_db).min() >= margin_db
    if min_peak_db is not None:
        assert np.abs(pk[np.isfinite(pk)] - min_peak_db).min() >= margin_db
    want = R.select(e, p, valids, *R.thresholds(min_rms_db, min_peak_db))
    got = ws.select(min_rms_db, min_peak_db).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (ws.n_windows + 1,)
    assert int(got[-1]) == len(want) and got[:len(want)].tolist() == want
    return want


def test_selection_matches_the_restatement(built_lib):
    x = _alternating()
    ws = recordings.windows(x, W_SEL / 16000, HOP_SEL / 16000)
    n = ws.n_windows
    assert n == 1250 and ws.valids[-4:].tolist() == [64, 48, 32, 16]
    assert _check_gate(ws, x, None, None) == list(range(n))                                      # all kept, the silent windows too
    assert _check_gate(ws, x, 20.0, None) == [] and _check_gate(ws, x, None, 6.0) == []          # none kept
    by_rms = _check_gate(ws, x, -40.0, None)                                                     # whatever holds any noise: across the 1 024 boundary
    assert 500 < len(by_rms) < 800 and by_rms[0] < 1024 < by_rms[-1]
    by_peak = _check_gate(ws, x, None, -6.0)                                                     # the windows that hold a spike: four each
    assert len(by_peak) == 4 * len(SPIKES) - 3 and by_peak[:2] == [0, 90]                        # (sample 0 is in window 0 alone)
    both = _check_gate(ws, x, -40.0, -6.0)
    assert both == sorted(set(by_rms) & set(by_peak)) == by_peak


def test_selection_of_a_single_window_first_and_last(built_lib):
    x = np.zeros(N_SEL, dtype=np.float32)
    x[0] = 1.0                                                                                   # sample 0 is in window 0 alone
    ws = recordings.windows(x, W_SEL / 16000, HOP_SEL / 16000)
    assert _check_gate(ws, x, None, -6.0) == [0] and _check_gate(ws, x, -30.0, -6.0) == [0]      # rms of window 0: 1 / 8 = -18.06 dB
    x = np.zeros(N_SEL, dtype=np.float32)
    x[N_SEL - 16:] = 1.0                                                                         # the last window's 16 samples; windows 1246 .. 1248 hold them too,
    x[N_SEL - 17] = np.nan                                                                       # and the NaN in front of them: never kept
    ws = recordings.windows(x, W_SEL / 16000, HOP_SEL / 16000)
    assert _check_gate(ws, x, None, -6.0) == [1249] and _check_gate(ws, x, -6.0, None) == [1249]
    assert np.isnan(ws.rms_db[1246:1249]).all() and ws.rms_db[1249] == 0.0


# ------------------------------------------------------------------------------------------------------------------------ 4. embeddings
WIN_S, HOP_S = 1.0, 0.37                                 # 16 000 and 5 920 samples: 14 windows over 5 s, the last one 3 040 samples


@pytest.fixture(scope="module")
def beats(built_lib):
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=2)
    m = avex_amd.beats_model.Model(device="cuda", init_config=cfg, return_features_only=True, batch_invariant=True).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.beats_state_dict(cfg, seed=0).items()}, strict=False)
    return m


@pytest.fixture(scope="module")
def clip():
    x = synth.noise_clips(1, 80000, seed=23)[0]
    gap = x.copy()
    gap[32000:48000] = 0.0                                # the middle second is zeros
    return x, gap


@pytest.fixture(scope="module")
def ungated(beats, clip):
    """The 14 embeddings of the clip with the silent middle, computed once: batch_size 256."""
    return recordings.embed_recording(beats, clip[1], WIN_S, HOP_S, layers=["last_layer"], batch_invariant=True)


def test_embeddings_do_not_depend_on_the_batch_size(beats, clip):
    x = clip[0]
    a = recordings.embed_recording(beats, x, WIN_S, HOP_S, layers=["last_layer"], batch_size=3, batch_invariant=True)
    b = recordings.embed_recording(beats, x, WIN_S, HOP_S, batch_size=256, batch_invariant=True)       # layers=None: what is registered
    ws = recordings.windows(x, WIN_S, HOP_S)
    assert ws.n_windows == 14 and ws.valids[-1] == 3040
    wav, mask = ws.batch(0, 14)
    direct = beats.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation="mean")
    assert direct.shape == (14, 768) and a["embeddings"].is_cuda and bool(torch.isfinite(direct).all())
    assert torch.equal(a["embeddings"], direct) and torch.equal(b["embeddings"], direct)
    assert len({tuple(r) for r in direct.cpu().numpy().round(4).tolist()}) == 14                 # fourteen different windows, fourteen different rows
    for r in (a, b):
        assert r["window_index"].tolist() == list(range(14)) and r["window_index"].dtype == torch.int64 and bool(r["kept"].all())
        assert np.array_equal(r["start_s"], ws.start_s) and np.array_equal(r["end_s"], ws.end_s)
        assert np.allclose(r["rms_db"].cpu().numpy(), ws.rms_db, rtol=0, atol=1e-9)              # log10 on the device and in NumPy may differ in the last bits
        assert np.allclose(r["peak_db"].cpu().numpy(), ws.peak_db, rtol=0, atol=1e-9) and r["rms_db"].dtype == torch.float64 and r["rms_db"].is_cuda
    frames = recordings.embed_recording(beats, x, WIN_S, HOP_S, aggregation="none", batch_size=5, batch_invariant=True)["embeddings"]
    assert frames.shape[0] == 14 and frames.shape[2] == 768 and frames.dim() == 3


def test_gate_keeps_the_ungated_bits(beats, clip, ungated):
    gap = clip[1]
    starts, valids = R.plan(80000, 16000, 5920)
    rms, _ = R.db(*R.stats(gap, starts, valids), valids)
    thr = float(rms[0]) - 4.5                             # 4.5 dB under a full window of noise: a window that is 65 % silence or more goes
    want = [w for w in range(14) if rms[w] >= thr]
    assert want == [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13] and np.abs(rms - thr).min() >= 1.0   # rounding of an fp64 sum moves rms_db by ~1e-14 dB
    g = recordings.embed_recording(beats, gap, WIN_S, HOP_S, batch_size=5, min_rms_db=thr, batch_invariant=True)
    assert g["window_index"].tolist() == want and g["kept"].tolist() == [w in want for w in range(14)]
    assert g["embeddings"].shape == (len(want), 768) and torch.equal(g["embeddings"], ungated["embeddings"][g["window_index"]])
    assert np.array_equal(g["start_s"], np.array(starts)[want] / 16000.0) and np.array_equal(g["end_s"], (np.array(starts) + np.array(valids))[want] / 16000.0)
    assert torch.equal(g["rms_db"], ungated["rms_db"]) and g["rms_db"].shape == (14,) and g["peak_db"].shape == (14,)
    none = recordings.embed_recording(beats, gap, WIN_S, HOP_S, min_rms_db=0.0, min_peak_db=-1.0, batch_invariant=True)
    assert none["embeddings"].shape[0] == 0 and none["window_index"].numel() == 0 and not none["kept"].any() and len(none["start_s"]) == 0


def test_recordings_share_batches_and_keep_their_bits(beats, clip, ungated):
    gap = clip[1]
    y = synth.normal("rec2", (88200, 1), 0.2).astype(np.float32).clip(-0.99, 0.99)
    other = _wav16(y, 44100)                              # 2 s at 44.1 kHz: 32 000 samples, 6 windows
    single = recordings.embed_recording(beats, other, WIN_S, HOP_S, batch_invariant=True)
    assert single["embeddings"].shape == (6, 768)
    for kw in ({}, {"min_rms_db": float(ungated["rms_db"][0]) - 4.5}):
        a, b = recordings.embed_recordings(beats, [other, gap], WIN_S, HOP_S, batch_size=4, batch_invariant=True, **kw)
        sa = recordings.embed_recording(beats, other, WIN_S, HOP_S, batch_invariant=True, **kw)
        sb = recordings.embed_recording(beats, gap, WIN_S, HOP_S, batch_invariant=True, **kw)
        for got, want in ((a, sa), (b, sb)):
            assert torch.equal(got["embeddings"], want["embeddings"]) and torch.equal(got["window_index"], want["window_index"])
            assert torch.equal(got["rms_db"], want["rms_db"]) and torch.equal(got["peak_db"], want["peak_db"]) and torch.equal(got["kept"], want["kept"])
            assert np.array_equal(got["start_s"], want["start_s"]) and np.array_equal(got["end_s"], want["end_s"])
        assert b["embeddings"].shape[0] == (12 if kw else 14) and torch.equal(sa["embeddings"], single["embeddings"])
    assert torch.equal(sb["embeddings"], ungated["embeddings"][sb["window_index"]])


def test_nothing_is_beats_specific(built_lib, tmp_path):
    from safetensors.numpy import save_file
    sd = synth.effnet_b0_state_dict()
    path = tmp_path / "effnet.safetensors"
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items() if not k.endswith("num_batches_tracked")}, str(path))
    m = avex_amd.load_model("esp_aves2_effnetb0_all", device="cuda", checkpoint_path=str(path), return_features_only=True).eval()
    x = synth.noise_clips(1, 40000, seed=29)[0]
    r = recordings.embed_recording(m, x, 1.0, 0.5)                                               # layers=None and nothing registered: the last layer
    ws = recordings.windows(x, 1.0, 0.5)
    assert ws.n_windows == 5 and m._hook_layers == ["model.features.8.0"]
    wav, mask = ws.batch(0, 5)
    direct = m.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation="mean")
    assert r["embeddings"].shape == direct.shape and direct.shape[0] == 5 and torch.equal(r["embeddings"], direct)
    m.deregister_all_hooks()


# ------------------------------------------------------------------------------------------------------------------------ 5. errors
def test_refusals(built_lib):
    x = synth.normal("recerr", (5000,), 0.1).astype(np.float32)
    with pytest.raises(ValueError, match="split the file"):
        recordings.windows(x, 0.1, max_resident_samples=4999)
    with pytest.raises(ValueError, match="split the file"):
        recordings.windows(_file_441(), 0.1, max_resident_samples=18140)                         # counted at the target rate
    assert recordings.windows(x, 0.1, max_resident_samples=5000).n_windows == 4
    with pytest.raises(ValueError):
        recordings.windows(x, 0.1, tail="keep")
    with pytest.raises(ValueError):
        recordings.windows(x, 0.1, 0.0)
    lib = _capi.lib()
    wav = torch.from_numpy(x).cuda()
    out = torch.full((3, 1000), 7.0, device="cuda")
    mask = torch.full((3, 1000), 7, dtype=torch.uint8, device="cuda")
    stat_e = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    stat_p = torch.full((3,), 7.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def gather(rows, first=0, B=3, index=None, window_len=1000, wav_samples=5000):
        tab, dev = _table(rows)
        rc = lib.avexhip_window_gather(wav.data_ptr(), wav_samples, tab.ctypes.data, dev.data_ptr(), len(rows), index, first, B, window_len, out.data_ptr(), 0,
                                       mask.data_ptr(), stream)
        return rc, _capi.last_error()

    good = [(0, 5000, 0, 1000), (0, 5000, 2000, 1000), (0, 5000, 4500, 500)]
    rc, msg = gather(good[:2] + [(0, 5000, 4500, 501)])                                          # one sample past the recording's end
    assert rc == -1 and "window 2" in msg and "leaves the recording" in msg
    tab, dev = _table(good[:2] + [(0, 5000, 4500, 501)])
    rc = lib.avexhip_window_stats(wav.data_ptr(), 5000, tab.ctypes.data, dev.data_ptr(), 3, 1000, stat_e.data_ptr(), stat_p.data_ptr(), stream)
    assert rc == -1 and "window 2" in _capi.last_error()
    idx = torch.zeros(3, dtype=torch.int32, device="cuda")
    refused = [gather([good[0], (0, 5000, -1, 1000), good[2]]), gather([good[0], (0, 5000, 0, 1001), good[2]]), gather([good[0], good[1], (0, 5001, 0, 10)]),
               gather([(1, 5000, 0, 10)] + good[1:]), gather(good, first=1), gather(good, first=-1), gather(good, B=0), gather(good, window_len=0),
               gather(good, wav_samples=4999), gather(good[:2] + [(0, 5000, 4500, 501)], index=idx.data_ptr(), B=1)]      # an indexed gather checks the whole table
    for rc, msg in refused:
        assert rc == -1 and msg.startswith("window_gather"), (rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mask == 7).all()) and bool((stat_e == 7.0).all()) and bool((stat_p == 7.0).all())      # nothing was launched
    rc, msg = gather(good)                                                                       # the same call with a good table runs
    assert rc == 0, msg
    torch.cuda.synchronize()
    r_wav, r_mask = R.rows(x, [0, 2000, 4500], [1000, 1000, 500], 1000)
    assert np.array_equal(out.cpu().numpy(), r_wav) and np.array_equal(mask.cpu().numpy().astype(bool), r_mask)
