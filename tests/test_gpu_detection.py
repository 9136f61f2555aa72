"""Event detection on the device: avex_amd.detection over csrc/events.hip (avexhip_events_*), bit for bit against the NumPy restatement
(tests/_detection_ref.py) in every column but ``mean``, which is held to the first-order bound of an fp64 sum in any order.

1. edges: sequence lengths around the ballot word and the chunk, narrow and wide class counts, every rule;
2. carries across whole chunks, and many short sequences inside one chunk;
3. one sequence of 2^20 windows: many events, an event over hundreds of chunks, and one event over everything;
4. missing scores through row_of_window;  5. capacity;  6. invariance to the run, the stride and the dtype;  7. sigmoid thresholds;
8. end to end from waveforms, with a stub model and with the synthetic BEATs encoder and a linear probe.
"""
import math

import numpy as np
import pytest
import torch

import _detection_ref as D
import avex_amd
from avex_amd import _capi, detection, probes, recordings, synth
from avex_amd.base_model import ModelBase

pytestmark = pytest.mark.gpu

INT_COLS = ("sequence", "class_id", "first", "last", "peak_window")


def _K():
    return int(_capi.lib().avexhip_events_chunk_windows())


def _host(res):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def _ar(name, n, c, coef):
    """y[t] = coef * y[t - 1] + e[t], rounded to quarters: ties, and sums that are exact in fp32 and fp64.  The noise has a standard
    deviation of 3, so that thresholds of 0 and 1 are crossed often: short gaps and short runs exist even behind a smoothing."""
    e = synth.normal(name, (n, c), 3.0).astype(np.float64)
    y = np.zeros((n, c))
    for t in range(n):
        y[t] = (coef * y[t - 1] if t else 0.0) + e[t]
    return (np.round(y * 4.0) / 4.0).astype(np.float32)


def _assert_events(got, want, terms, what=""):
    """Every column exact, mean within n * 2^-52 * (sum |x| / n) of math.fsum."""
    n = len(want["first"])
    assert int(got["count"]) == n, (what, int(got["count"]), n)
    for key in INT_COLS:
        g = got[key][:n]
        assert g.dtype == np.int32 and np.array_equal(g, want[key]), (what, key, np.flatnonzero(g != want[key])[:5])
    assert got["peak"].dtype == np.float32 and np.array_equal(got["peak"][:n].view(np.int32), want["peak"].view(np.int32)), (what, "peak")
    assert np.array_equal(got["n_windows"][:n], want["last"] - want["first"] + 1), (what, "n_windows")
    assert got["mean"].dtype == np.float64
    for j in range(n):
        assert abs(got["mean"][j] - want["mean"][j]) <= D.mean_bound(terms[j]), (what, "mean", j, got["mean"][j], want["mean"][j])


def _assert_same_bits(a, b, what=""):
    assert set(a) == set(b), what
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key)


def _decode_both(x, offsets, rule, **kw):
    smooth, mode, gap, minw = rule
    st = {}
    want = D.decode(x, offsets, 1.0, 0.0, smooth=smooth, smooth_mode=mode, merge_gap=gap, min_windows=minw, stats=st)
    got = _host(detection.decode_events(x, seq_offsets=offsets, on=1.0, off=0.0, smooth=smooth, smooth_mode=mode, merge_gap=gap, min_windows=minw, **kw))
    return got, want, st


# ------------------------------------------------------------------------------------------------------------------ 1. edges
RULES = [(1, "median", 0, 1), (1, "median", 2, 3), (5, "median", 2, 3), (5, "mean", 1, 2), (31, "mean", 64, 64)]


@pytest.mark.parametrize("rule", RULES, ids=[f"s{r[0]}{r[1]}-g{r[2]}-m{r[3]}" for r in RULES])
@pytest.mark.parametrize("c", [1, 3, 65])
def test_edges(built_lib, c, rule):
    K = _K()
    coef = 0.8 if rule[0] == 31 else 0.5
    lengths = (1, 2, 63, 64, 65, K - 1, K, K + 1, 3 * K + 5)
    singles = []
    raw = merged = kept = 0
    for n in lengths:
        x = _ar(f"det-edge-{n}-{c}-{coef}", n, c, coef)
        got, want, st = _decode_both(x, [0, n], rule)
        _assert_events(got, want, st["mean_terms"], f"n={n}")
        assert len(got["first"]) == len(want["first"])                                   # max_events=None allocates exactly
        if n >= 255:
            raw, merged, kept = raw + st["raw"], merged + st["merged"], kept + st["kept"]
        singles.append((x, want, st["mean_terms"]))
    # the restatement itself merged a gap and dropped a run in the sequences of 255 windows and more.  Counted over those sequences
    # together: one class over 255 windows behind a 31-window mean has one or two runs, so no recipe gives every sequence both
    if rule[2] > 0:
        assert merged < raw, (raw, merged)
    if rule[3] > 1:
        assert kept < merged, (merged, kept)
    # the same sequences back to back (boundaries inside words and chunks), two of them empty: each sequence's events, shifted
    offsets = np.concatenate([[0, 0], np.cumsum(lengths)[:4], [int(np.cumsum(lengths)[3])], np.cumsum(lengths)[4:]]).astype(np.int64)
    seq_of = [1, 2, 3, 4, 6, 7, 8, 9, 10]
    want = {k: [] for k in D.FIELDS}
    terms = []
    for r, (x, w, t) in zip(seq_of, singles):
        shift = int(offsets[r])
        for k in D.FIELDS:
            col = w[k]
            want[k].append(np.full_like(col, r) if k == "sequence" else col + shift if k in ("first", "last", "peak_window") else col)
        terms += t
    want = {k: np.concatenate(v) for k, v in want.items()}
    smooth, mode, gap, minw = rule
    got = _host(detection.decode_events(np.concatenate([s[0] for s in singles]), seq_offsets=offsets, on=1.0, off=0.0, smooth=smooth, smooth_mode=mode,
                                        merge_gap=gap, min_windows=minw))
    _assert_events(got, want, terms, "packed")


# ------------------------------------------------------------------------------------------------------------------ 2. carries
def test_state_is_carried_across_whole_chunks(built_lib):
    K = _K()
    x = np.full((3 * K + 2, 1), 0.5, dtype=np.float32)                                    # holds ...
    x[0], x[-1] = 2.0, -1.0                                                               # ... between a set and a clear
    got = _host(detection.decode_events(x, on=1.0, off=0.0))
    assert int(got["count"]) == 1 and (got["first"].tolist(), got["last"].tolist()) == ([0], [3 * K]) and got["sequence"].tolist() == [0]
    assert got["peak"].tolist() == [2.0] and got["peak_window"].tolist() == [0]
    vals = [2.0] + [0.5] * (3 * K)
    assert abs(got["mean"][0] - math.fsum(vals) / len(vals)) <= D.mean_bound(vals)
    x[0] = 0.5                                                                            # the set replaced by a hold: nothing to carry
    got = _host(detection.decode_events(x, on=1.0, off=0.0))
    assert int(got["count"]) == 0 and got["first"].shape == (0,)
    x[K + 3] = 2.0                                                                        # a set inside the second chunk, a merge and a minimum on top
    got = _host(detection.decode_events(x, on=1.0, off=0.0, merge_gap=5, min_windows=64))
    assert (got["first"].tolist(), got["last"].tolist()) == ([K + 3], [3 * K])


def test_more_chunks_than_one_pass_of_the_count(built_lib):
    """One class over 256 chunks and one window: the prefix of the event starts over the chunks takes a second pass of 256 with the
    first pass's total as its carry.  Sparse events, one of them across the last chunk boundary."""
    K = _K()
    n = 256 * K + 1
    x = np.full((n, 1), 0.5, dtype=np.float32)                                            # holds ...
    starts = np.arange(37, n - 1000, 997)
    x[starts], x[starts + 5] = 2.0, -1.0                                                  # ... between sets and clears five windows later,
    x[starts[::3] + 2] = 2.25                                                             # a peak behind the first window in every third event
    x[256 * K - 2] = 2.0                                                                  # and a set that no clear follows: windows 256 K - 2 .. 256 K
    got, want, st = _decode_both(x, [0, n], (1, "median", 0, 1))
    _assert_events(got, want, st["mean_terms"])
    assert len(want["first"]) == len(starts) + 1 > 64 and (want["first"][-1], want["last"][-1]) == (256 * K - 2, 256 * K)
    assert np.array_equal(want["last"][:-1], starts + 4) and want["peak_window"][0] == starts[0] + 2


def test_many_short_sequences_share_a_chunk(built_lib):
    lengths = [1 + (7 * j) % 40 for j in range(200)]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    x = _ar("det-short", int(offsets[-1]), 2, 0.5)
    for j, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        x[lo, :] = 0.5                                                                    # every sequence starts on a hold ...
        if j % 2 == 0:
            x[hi - 1, :] = 2.0                                                            # ... and every second one ends active
    rule = (1, "median", 1, 1)
    got, want, st = _decode_both(x, offsets, rule)
    _assert_events(got, want, st["mean_terms"], "packed")
    assert st["kept"] >= 200 and st["merged"] < st["raw"]
    on_first = want["first"] == offsets[want["sequence"]]                                 # a sequence's first window holds: no event starts there ...
    assert (np.asarray(lengths)[want["sequence"][on_first]] == 1).all()                   # ... but in the sequences of one window, which is the set
    alone = {k: [] for k in ("sequence", "class_id", "first", "last", "peak_window", "peak", "mean")}
    for j, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):                         # one sequence per call: the same events, shifted
        one = _host(detection.decode_events(x[lo:hi], on=1.0, off=0.0, merge_gap=1))
        for k in alone:
            alone[k].append(one[k] + (j if k == "sequence" else int(lo) if k in ("first", "last", "peak_window") else 0))
    for k in alone:
        a = np.concatenate(alone[k])
        assert a.dtype == got[k].dtype and np.array_equal(a, got[k]), k                   # quarters: the means are exact, so they are equal too


# ------------------------------------------------------------------------------------------------------------------ 3. long
def test_one_long_sequence(built_lib):
    n, period = 1 << 20, 4096
    i = np.arange(n)
    x = np.full(n, 0.5, dtype=np.float32)
    x[i % period == 0] = 2.0                                                              # a set every 4 096 windows ...
    x[i % period == 100] = -1.0                                                           # ... a clear 100 windows later
    p = i // period
    x[(p >= 100) & (p < 140) & (i % period == 100)] = 0.5                                 # holds across the middle: the event of period 100 ...
    x[(p > 100) & (p < 140) & (i % period == 0)] = 0.5                                    # ... runs to the clear of period 140
    xd = torch.from_numpy(x[:, None]).cuda()
    got = _host(detection.decode_events(xd, on=1.0, off=0.0))
    periods = np.concatenate([np.arange(0, 101), np.arange(141, n // period)])      # the set of period 140 is inside the long event
    first = periods * period
    last = first + 99
    last[100] = 140 * period + 99
    m = len(first)
    assert int(got["count"]) == m == 216 and got["first"].shape == (m,)
    assert np.array_equal(got["first"], first) and np.array_equal(got["last"], last) and np.array_equal(got["peak_window"], first)
    assert (got["peak"] == 2.0).all() and (got["sequence"] == 0).all() and (got["class_id"] == 0).all()
    length = (last - first + 1).astype(np.float64)
    total = 2.0 + 0.5 * (length - 1.0)                                                    # exact: multiples of a half
    total[100] = 2.0 + 0.5 * (length[100] - 2.0) + 2.0                                    # the long event also holds the set of period 140
    bound = length * 2.0 ** -52 * (total / length)
    assert (np.abs(got["mean"] - total / length) <= bound).all()
    # everything one event: every value but the clears sets, the clears hold
    got = _host(detection.decode_events(xd, on=0.25, off=-2.0))
    assert int(got["count"]) == 1 and got["first"].tolist() == [0] and got["last"].tolist() == [n - 1]
    assert got["peak"].tolist() == [2.0] and got["peak_window"].tolist() == [0]
    s = float(x.astype(np.float64).sum())                                                 # exact: multiples of a half below 2^53
    assert abs(got["mean"][0] - s / n) <= n * 2.0 ** -52 * (float(np.abs(x).astype(np.float64).sum()) / n)


# ------------------------------------------------------------------------------------------------------------------ 4. missing scores
def test_missing_scores_and_permuted_rows(built_lib):
    K = _K()
    n, c = 2 * K + 37, 5
    full = _ar("det-miss", n, c, 0.8)
    full[np.arange(n) % 3 == 1] = np.nan                                                  # every third window has no score
    offsets = [0, 100, n]
    have = np.flatnonzero(~np.isnan(full[:, 0]))
    perm = np.argsort(synth.normal("det-perm", (len(have),), 1.0), kind="stable")          # the score rows in another order
    row_of_window = np.full(n, -1, dtype=np.int64)
    row_of_window[have[perm]] = np.arange(len(have))
    rows = full[have[perm]]
    for rule in ((1, "median", 2, 2), (5, "median", 2, 3), (5, "mean", 1, 2)):
        smooth, mode, gap, minw = rule
        got_nan, want, st = _decode_both(full, offsets, rule)
        _assert_events(got_nan, want, st["mean_terms"], f"nan {rule}")
        assert st["kept"] > 0
        got = _host(detection.decode_events(rows, seq_offsets=offsets, on=1.0, off=0.0, smooth=smooth, smooth_mode=mode, merge_gap=gap, min_windows=minw,
                                            row_of_window=torch.from_numpy(row_of_window).cuda()))
        _assert_same_bits(got, got_nan, f"rows {rule}")


# ------------------------------------------------------------------------------------------------------------------ 5. capacity
def test_capacity(built_lib):
    x = _ar("det-cap", 1000, 3, 0.5)
    offsets = [0, 400, 1000]
    full = _host(detection.decode_events(x, seq_offsets=offsets, on=1.0, off=0.0, merge_gap=1))
    n = int(full["count"])
    assert n > 50 and all(v.shape == (n,) for k, v in full.items() if k != "count")
    for cap in (0, 1, 17, n - 1, n, n + 9):
        got = _host(detection.decode_events(x, seq_offsets=offsets, on=1.0, off=0.0, merge_gap=1, max_events=cap))
        assert int(got["count"]) == n, cap                                               # the true total, whatever was written
        k = min(cap, n)
        for key, v in got.items():
            if key == "count":
                continue
            assert v.shape == (cap,) and v[:k].tobytes() == full[key][:k].tobytes(), (cap, key)
            tail = v[k:]
            assert np.isnan(tail).all() if key == "mean" else np.isneginf(tail).all() if key == "peak" else (tail == -1).all(), (cap, key)


# ------------------------------------------------------------------------------------------------------------------ 6. invariance
def test_runs_strides_and_dtypes_give_the_same_bits(built_lib):
    K = _K()
    x = _ar("det-inv", K + 77, 20, 0.8)
    kw = dict(seq_offsets=[0, 50, K + 77], on=1.0, off=0.0, smooth=3, smooth_mode="mean", merge_gap=2, min_windows=2)
    a = _host(detection.decode_events(x, **kw))
    assert int(a["count"]) > 10
    _assert_same_bits(a, _host(detection.decode_events(x, **kw)), "run")
    wide = torch.full((K + 77, 33), 7.0, device="cuda")
    wide[:, 5:25] = torch.from_numpy(x).cuda()
    view = wide[:, 5:25]
    assert view.stride(0) == 33 and not view.is_contiguous()
    _assert_same_bits(a, _host(detection.decode_events(view, **kw)), "stride")
    half = torch.from_numpy(x).cuda().to(torch.float16)                                   # quarters of moderate size are exact in f16
    assert torch.equal(half.to(torch.float32).cpu(), torch.from_numpy(x))
    _assert_same_bits(a, _host(detection.decode_events(half, **kw)), "f16")
    third = (torch.from_numpy(x).cuda() / 3.0).to(torch.float16)                          # values f16 rounds: the bits of their fp32 conversion
    _assert_same_bits(_host(detection.decode_events(third, **kw)), _host(detection.decode_events(third.to(torch.float32), **kw)), "f16 rounded")


# ------------------------------------------------------------------------------------------------------------------ 7. sigmoid
def test_sigmoid_thresholds_are_logits(built_lib):
    x = _ar("det-sig", 600, 4, 0.8)
    p_on, p_off = np.asarray([0.7, 0.6, 0.9, 0.5]), np.asarray([0.4, 0.6, 0.2, 0.1])
    on = np.log(p_on / (1.0 - p_on)).astype(np.float32)
    off = np.log(p_off / (1.0 - p_off)).astype(np.float32)
    want = _host(detection.decode_events(x, on=on, off=off, merge_gap=1))
    res = detection.decode_events(x, on=p_on, off=p_off, activation="sigmoid", merge_gap=1)
    got = _host(res)
    assert int(got["count"]) > 10 and torch.equal(res["peak_prob"], torch.sigmoid(res["peak"])) and res["peak_prob"].dtype == torch.float32
    got.pop("peak_prob")
    _assert_same_bits(got, want, "sigmoid")
    st = {}
    ref = D.decode(x, [0, 600], on, off, merge_gap=1, stats=st)
    _assert_events(got, ref, st["mean_terms"], "logits")


# ------------------------------------------------------------------------------------------------------------------ 8. end to end
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


BURSTS = ((10.0, 13.0), (25.5, 27.0), (40.0, 42.5))


def test_end_to_end_finds_the_pasted_bursts(built_lib):
    sr, hop = 16000, 0.5
    x = 0.001 * synth.normal("det-floor", (60 * sr,), 1.0)                                # a -60 dB floor ...
    for j, (t0, t1) in enumerate(BURSTS):
        a, b = int(t0 * sr), int(t1 * sr)
        x[a:b] = 0.1 * synth.normal(f"det-burst-{j}", (b - a,), 1.0)                      # ... and three bursts at -20 dB
    x = x.astype(np.float32).clip(-0.99, 0.99)
    w = torch.tensor([[0.1]], device="cuda")

    def probe(e):                                                                         # one weight: (rms_db + 40) / 10
        return (e + 40.0) @ w

    res = detection.detect_events(_RmsModel(), probe, [x, x[:20 * sr]], 1.0, hop, on=0.0, off=-1.0, min_rms_db=-50.0, return_scores=True)
    assert res["names"] == ["0", "1"] and res["scores"].shape[1] == 1 and res["row_of_window"].shape == (120 + 40,)
    assert int((res["row_of_window"] < 0).sum()) > 80                                     # the gate dropped the floor: those windows have no score
    got = _host(res)
    assert int(got["count"]) == 4 and got["recording"].tolist() == [0, 0, 0, 1] == got["sequence"].tolist()
    for j, (t0, t1) in enumerate(BURSTS + (BURSTS[0],)):
        assert got["start_s"][j] <= t0 <= got["start_s"][j] + hop and got["end_s"][j] - hop <= t1 <= got["end_s"][j], (j, got["start_s"][j], got["end_s"][j])
        assert got["start_s"][j] <= got["peak_s"][j] < got["end_s"][j] and got["start_s"].dtype == np.float64
    assert [res["names"][r] for r in got["recording"]] == ["0", "0", "0", "1"]
    ws = recordings.windows(x, 1.0, hop)
    assert np.array_equal(got["start_s"][:3], ws.start_s[got["first"][:3]]) and np.array_equal(got["end_s"][:3], ws.end_s[got["last"][:3]])
    again = _host(detection.decode_events(res["scores"], seq_offsets=[0, 120, 160], on=0.0, off=-1.0, row_of_window=res["row_of_window"]))
    for key in again:
        assert again[key].tobytes() == got[key].tobytes(), key
    ungated = _host(detection.detect_events(_RmsModel(), probe, [x], 1.0, hop, on=0.0, off=-1.0))      # without a gate: the same three events
    assert int(ungated["count"]) == 3 and np.array_equal(ungated["first"], got["first"][:3]) and np.array_equal(ungated["last"], got["last"][:3])


def test_end_to_end_with_an_encoder_and_a_linear_probe(built_lib):
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=2)
    m = avex_amd.beats_model.Model(device="cuda", init_config=cfg, return_features_only=True, batch_invariant=True).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.beats_state_dict(cfg, seed=0).items()}, strict=False)
    head = probes.LinearProbe(None, [], 3, device="cuda", feature_mode=True, input_dim=768)
    head.load_state_dict({"classifier.weight": torch.from_numpy(synth.normal("det-probe-w", (3, 768), 0.05).astype(np.float32)),
                          "classifier.bias": torch.zeros(3)})
    x = synth.noise_clips(1, 80000, seed=23)[0]
    x[32000:48000] = 0.0
    gate = float(np.median(recordings.windows(x, 1.0, 0.37).rms_db)) - 3.0                # drops the windows that are mostly the silent second
    first = detection.detect_events(m, head, [x], 1.0, 0.37, on=0.0, return_scores=True, min_rms_db=gate, layers=["last_layer"])
    scores = first["scores"]
    assert scores.shape == (int((first["row_of_window"] >= 0).sum()), 3) and 0 < scores.shape[0] < 14 == first["row_of_window"].shape[0]
    on = scores.median(0).values.cpu().numpy()                                            # thresholds that split the windows
    res = detection.detect_events(m, head, [x], 1.0, 0.37, on=on, off=on - 0.01, return_scores=True, min_rms_db=gate, merge_gap=1)
    assert torch.equal(res["scores"], scores) and int(res["count"]) >= 1
    again = detection.decode_events(res["scores"], seq_offsets=[0, 14], on=on, off=on - 0.01, merge_gap=1, row_of_window=res["row_of_window"])
    for key, v in again.items():
        assert torch.equal(v, res[key]) or key == "mean" and v.cpu().numpy().tobytes() == res[key].cpu().numpy().tobytes(), key
    m.deregister_all_hooks()
