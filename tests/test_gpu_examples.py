"""Few-shot class scores on the device: avex_amd.examples over csrc/examples.hip (avexhip_examples_*).

1. inputs whose products and sums are exact in fp32: scores and nearest equal the NumPy restatement (tests/_examples_ref.py) bit for bit,
   ties at the m-th place included, across tile, segment and batch edges, every list depth and both modes;
2. random fp32 rows: scores and nearest equal the restatement applied to the device's own similarities, taken from an EmbeddingIndex over
   the same rows -- the fused kernel runs the shared tile, not a copy of it;
3. scores do not depend on batch_size, on the pieces or the order the rows were added in, or on the run;
4. NaN and zero rows;
5. prototypes against the restatement on the device's own prepared rows;
6. a bank that went through state_dict answers with the same bits;
7. end to end: events from one annotated example of a segment pasted into a recording.
"""
import io

import numpy as np
import pytest
import torch

import _examples_ref as E
import _search_ref as S
import avex_amd
from avex_amd import detection, examples, search, synth

pytestmark = pytest.mark.gpu

TOP_MS = (1, 2, 5, 16)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"i{a.itemsize}") if a.dtype.kind == "f" else a


def _assert_same(got, want, what=""):
    """(scores, nearest) bit for bit; any NaN is "no number": its payload bits are not part of the contract."""
    (gs, gn), (ws, wn) = got, want
    gs, gn = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (gs, gn))
    assert gs.dtype == ws.dtype == np.float32 and gs.shape == ws.shape, (what, gs.dtype, gs.shape, ws.shape)
    assert gn.dtype == wn.dtype == np.int32 and gn.shape == wn.shape, (what, gn.dtype, gn.shape, wn.shape)
    nan = np.isnan(gs) & np.isnan(ws)
    assert np.array_equal(_bits(gs)[~nan], _bits(ws)[~nan]), (what, "scores", np.argwhere((_bits(gs) != _bits(ws)) & ~nan)[:5])
    assert np.array_equal(gn, wn), (what, "nearest", np.argwhere(gn != wn)[:5])


def _pm1(name, shape):
    return np.where(synth.normal(name, shape, 1.0) >= 0, 1.0, -1.0).astype(np.float32)


def _small_ints(name, shape):
    return np.clip(np.rint(synth.normal(name, shape, 1.5)), -3, 3).astype(np.float32)


def _labels(counts, seed):
    """Labels with the given rows per class (the background last), in a shuffled order: the order of adding is not the sorted one."""
    c = len(counts) - 1
    lab = np.repeat(np.arange(c + 1), counts)
    lab[lab == c] = -1
    return lab[np.random.RandomState(seed).permutation(len(lab))]


def _device_sim(rows, q, metric):
    """The device's own similarities [nq, n], from an unmodified EmbeddingIndex over the same rows."""
    ix = search.EmbeddingIndex(rows.shape[1], metric=metric, chunk_rows=4096)
    ix.add(rows)
    return ix.search(q, 1, return_sim=True)["sim"].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ 1. exact arithmetic
#         metric    d    rows per class ..., background                      N    batch_size
EXACT = [("cosine", 16, (1, 0), 1, 1),                                                       # one row
         ("cosine", 256, (128, 0), 127, 128),                                                # a class ending exactly on the tile edge, no background
         ("dot", 33, (100, 25, 3, 1), 129, 128),                                             # ... with the background alone in the next tile
         ("dot", 768, (0, 50, 300, 0, 3, 0, 32), 300, 4096),                                 # a class over three tiles; empty classes first, amid, last
         ("cosine", 16, (1,) * 128 + (1,), 300, 128),                                        # 128 one-row classes in one tile
         ("dot", 33, (3, 200, 182), 127, 1),                                                 # classes and background over tile edges, one window a batch
         ("cosine", 256, (60, 7, 200, 118), 129, 4096)]


@pytest.mark.parametrize("metric,d,counts,n,batch_size", EXACT, ids=[f"{c[0]}-d{c[1]}-m{sum(c[2])}-c{len(c[2]) - 1}-n{c[3]}-b{c[4]}" for c in EXACT])
def test_exact_arithmetic_exact_scores(built_lib, metric, d, counts, n, batch_size):
    """+-1 entries with d in {16, 256} (norms 4, 16) and integers |x| <= 3: every similarity, every sum of at most 16 of them and their
    order are exact in fp32, so the scores are known without a tolerance."""
    make = _pm1 if metric == "cosine" else _small_ints
    m, c = sum(counts), len(counts) - 1
    rows, q = make(f"ex-db-{d}-{m}", (m, d)), make(f"ex-q-{d}-{n}", (n, d))
    labels = _labels(counts, m)
    sim = S.prepared(q, metric) @ S.prepared(rows, metric).T
    assert np.array_equal(sim.astype(np.float64), S.prepared(q, metric).astype(np.float64) @ S.prepared(rows, metric).astype(np.float64).T)      # exact indeed
    bank = examples.ExampleBank(d, n_classes=c, metric=metric)
    assert bank.add(rows, labels) == range(0, m) and len(bank) == m and bank.counts.tolist() == list(counts)
    ties = short = 0
    for top_m in TOP_MS:
        for cl in range(c):
            s = np.sort(sim[:, labels == cl], axis=1)[:, ::-1]
            if s.shape[1] > top_m:
                ties += int((s[:, top_m - 1] == s[:, top_m]).sum())                         # the m-th and the (m + 1)-th largest are equal
            short += int(0 < s.shape[1] < top_m)
        for mode in ("similarity", "margin") if counts[-1] else ("similarity",):
            got = bank.score(torch.from_numpy(q).cuda() if top_m == 2 else q, top_m=top_m, mode=mode, batch_size=batch_size, return_nearest=True)
            _assert_same(got, E.score(sim, labels, c, top_m, mode), f"top_m={top_m} {mode}")
            only = bank.score(q, top_m=top_m, mode=mode, batch_size=batch_size)
            assert isinstance(only, torch.Tensor) and only.is_cuda and torch.equal(only.view(torch.int32), got[0].view(torch.int32))
    if max(counts[:-1]) > 16 and 0 < min(k for k in counts[:-1] if k) < 16:                # a class deeper than every list beside a short one
        assert ties > 0 and short > 0, (ties, short)                                        # ties at the m-th place; a class with fewer than top_m rows


# ------------------------------------------------------------------------------------------------------------------ 2. random rows
N_RAND, CLASSES, N_BG = 300, 40, 400


def _random_bank(d, extra_empty=0):
    """1 500 rows over 40 uneven classes (the smallest hold one to three rows) and 400 background rows, in a shuffled order."""
    rng = np.random.RandomState(11)
    counts = 1 + rng.multinomial(1500 - CLASSES, rng.dirichlet(np.full(CLASSES, 0.7)))
    assert counts.sum() == 1500 and counts.min() <= 3 and counts.max() > 128
    counts = list(counts) + [0] * extra_empty + [N_BG]
    rows = synth.normal(f"ex-rand-db-{d}", (1500 + N_BG, d), 1.0).astype(np.float32)
    q = synth.normal(f"ex-rand-q-{d}", (N_RAND, d), 1.0).astype(np.float32)
    return rows, _labels(counts, 5), q, len(counts) - 1


@pytest.fixture(scope="module")
def rand40(built_lib):
    """The random bank of width 40 under cosine with the device's own similarities: shared, and left unchanged, by the tests below."""
    rows, labels, q, c = _random_bank(40)
    return {"rows": rows, "labels": labels, "q": q, "c": c, "sim": _device_sim(rows, q, "cosine")}


@pytest.mark.parametrize("metric,d", [("cosine", 40), ("dot", 40), ("cosine", 768), ("dot", 768)])
def test_random_rows_against_the_devices_own_similarities(built_lib, metric, d):
    rows, labels, q, c = _random_bank(d)
    sim = _device_sim(rows, q, metric)
    assert sim.shape == (N_RAND, 1900) and np.isfinite(sim).all()
    bank = examples.ExampleBank(d, metric=metric)
    bank.add(torch.from_numpy(rows).cuda(), labels)
    assert bank.n_classes == c == CLASSES and int(bank.counts[-1]) == N_BG
    for top_m, mode in ((1, "similarity"), (5, "margin"), (16, "similarity"), (3, "margin")):
        got = bank.score(torch.from_numpy(q).cuda(), top_m=top_m, mode=mode, batch_size=128, return_nearest=True)
        _assert_same(got, E.score(sim, labels, c, top_m, mode), f"{metric} d={d} top_m={top_m} {mode}")
    near = got[1].cpu().numpy()
    assert (labels[near] == np.arange(c)[None, :]).all()                                    # the nearest row of a class is of that class


# ------------------------------------------------------------------------------------------------------------------ 3. invariance
def test_scores_do_not_depend_on_batches_pieces_order_or_the_run(rand40):
    rows, labels, q, c, sim = (rand40[k] for k in ("rows", "labels", "q", "c", "sim"))
    for cl in range(c):                                                                     # distinct where nearest looks: the largest similarity of
        top2 = np.sort(sim[:, labels == cl], axis=1)[:, -2:]                                # every (window, class) is attained once (1 900 fp32 cosines of
        assert top2.shape[1] == 1 or (top2[:, 0] < top2[:, 1]).all(), cl                    # one window do collide somewhere: a row of them is not all distinct)
    m = len(rows)
    perm = np.random.RandomState(23).permutation(m)
    base = None
    for pieces, order, batch_size in (((m,), None, 4096), ((1, 130, 7, 256, 606, 900), None, 100), ((m,), perm, 1), ((999, 901), perm, 4096)):
        r, l = (rows, labels) if order is None else (rows[order], labels[order])
        bank = examples.ExampleBank(40)
        lo = 0
        for p in pieces:
            assert bank.add(r[lo:lo + p], l[lo:lo + p]) == range(lo, lo + p)
            lo += p
        assert lo == m == len(bank)
        runs = [bank.score(q, top_m=5, mode="margin", batch_size=batch_size, return_nearest=True) for _ in range(2)]
        runs = [(s.cpu().numpy(), nr.cpu().numpy()) for s, nr in runs]
        if order is not None:                                                               # row i of this bank is row order[i] of the first
            runs = [(s, order[nr].astype(np.int32)) for s, nr in runs]
        what = f"pieces={pieces} permuted={order is not None} batch_size={batch_size}"
        _assert_same(runs[1], runs[0], what + " second run")
        if base is None:
            base = runs[0]
            _assert_same(base, E.score(sim, labels, c, 5, "margin"), "base")
        _assert_same(runs[0], base, what)


# ------------------------------------------------------------------------------------------------------------------ 4. NaN and zero rows
def test_nan_and_zero_rows(built_lib):
    d = 32
    rows = synth.normal("ex-nan-db", (12, d), 1.0).astype(np.float32)
    labels = np.array([0, 0, 0, 1, 1, 1, 2, -1, -1, 0, 1, -1])
    rows[1, 5] = np.nan                                                                     # a NaN row in class 0
    rows[4] = 0.0                                                                           # a zero row in class 1
    rows[6, 0] = np.nan                                                                     # class 2 holds a NaN row and nothing else
    q = synth.normal("ex-nan-q", (5, d), 1.0).astype(np.float32)
    q[1, 3] = np.nan
    q[3] = 0.0
    sim = _device_sim(rows, q, "cosine")
    assert np.isnan(sim[:, 1]).all() and np.isnan(sim[:, 6]).all() and np.isnan(sim[1]).all() and (sim[[0, 2, 4], 4] == 0).all() and (sim[3, [0, 2, 3]] == 0).all()
    bank = examples.ExampleBank(d)
    bank.add(rows, labels)
    clean = examples.ExampleBank(d, n_classes=3)
    keep = ~np.isnan(rows).any(axis=1)
    clean.add(rows[keep], labels[keep])
    for top_m in (1, 3, 16):
        for mode in ("similarity", "margin"):
            got = bank.score(q, top_m=top_m, mode=mode, return_nearest=True)
            _assert_same(got, E.score(sim, labels, 3, top_m, mode), f"top_m={top_m} {mode}")
            s, near = got[0].cpu().numpy(), got[1].cpu().numpy()
            assert np.isnan(s[1]).all() and (near[1] == -1).all()                           # a NaN window: a NaN row of scores, no nearest
            assert np.isnan(s[:, 2]).all() and (near[:, 2] == -1).all()                     # a class of NaN rows only
            assert np.isfinite(s[[0, 2, 3, 4]][:, :2]).all() and not (near == 1).any() and not (near == 6).any()
            assert (s[3, :2] == 0).all() and near[3].tolist() == [0, 3, -1]                 # a zero window ties everywhere: the lowest row of the class
            other = clean.score(q, top_m=top_m, mode=mode).cpu().numpy()                    # the NaN rows are ignored by their class
            assert np.array_equal(_bits(other)[~np.isnan(other)], _bits(s)[~np.isnan(s)]) and np.array_equal(np.isnan(other), np.isnan(s))


# ------------------------------------------------------------------------------------------------------------------ 5. prototypes
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_prototypes(built_lib, metric):
    d = 40
    rows, labels, q, c = _random_bank(d, extra_empty=2)                                     # classes 40 and 41 are empty
    assert c == 42
    bank = examples.ExampleBank(d, n_classes=c, metric=metric, class_names=[f"s{i}" for i in range(c)])
    bank.add(rows[:700], labels[:700])
    bank.add(torch.from_numpy(rows[700:]).cuda(), labels[700:])
    proto = bank.prototypes()
    assert len(proto) == 41 and proto.n_classes == c and proto.metric == metric and proto.class_names == bank.class_names and len(bank) == 1900
    assert proto.labels.tolist() == list(range(40)) + [-1] and proto.counts.tolist() == [1] * 40 + [0, 0, 1]
    means, lab = E.prototypes(bank.state_dict()["rows"], labels, c)                         # on the device's own prepared rows
    assert lab.tolist() == proto.labels.tolist()
    ix = search.EmbeddingIndex(d, metric=metric)                                            # the means, prepared again by the shared code
    ix.add(means)
    assert np.array_equal(_bits(proto.state_dict()["rows"]), _bits(ix.state_dict()["rows"]))
    if metric == "dot":
        assert np.array_equal(_bits(proto.state_dict()["rows"]), _bits(means))
    sim = ix.search(q, 1, return_sim=True)["sim"].cpu().numpy()
    for mode in ("similarity", "margin"):                                                   # nearest-prototype scoring
        got = proto.score(q, top_m=1, mode=mode, batch_size=100, return_nearest=True)
        _assert_same(got, E.score(sim, lab, c, 1, mode), mode)
        assert np.isnan(got[0][:, 40:].cpu().numpy()).all() and np.isfinite(got[0][:, :40].cpu().numpy()).all()
    assert len(examples.ExampleBank(d).prototypes()) == 0


# ------------------------------------------------------------------------------------------------------------------ 6. state
def test_state_dict_round_trip_gives_the_same_bits(rand40):
    rows, labels, q = rand40["rows"], rand40["labels"], rand40["q"]
    bank = examples.ExampleBank(40, n_classes=45, class_names=[f"s{i}" for i in range(45)])
    bank.add(rows, labels)
    buf = io.BytesIO()
    np.savez(buf, **bank.state_dict())
    buf.seek(0)
    back = examples.ExampleBank.from_state_dict(dict(np.load(buf)))
    assert len(back) == len(bank) and back.metric == bank.metric and back.n_classes == 45 and back.class_names == bank.class_names
    st0, st1 = bank.state_dict(), back.state_dict()
    assert sorted(st0) == sorted(st1)
    for key in st0:
        a, b = st0[key], st1[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    for kw in (dict(top_m=1), dict(top_m=7, mode="margin")):
        a = bank.score(q, return_nearest=True, **kw)
        b = back.score(q, return_nearest=True, **kw)
        _assert_same(b, (a[0].cpu().numpy(), a[1].cpu().numpy()), str(kw))


# ------------------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.fixture(scope="module")
def beats(built_lib):
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=2)
    m = avex_amd.beats_model.Model(device="cuda", init_config=cfg, return_features_only=True, batch_invariant=True).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.beats_state_dict(cfg, seed=0).items()}, strict=False)
    return m


def test_events_from_one_annotated_example(beats):
    sr, W = 16000, 16000
    x = synth.noise_clips(1, 10 * W, seed=31)[0].copy()
    seg = synth.noise_clips(1, W, seed=41)[0]
    at = [2, 4, 7, 9]
    for w in at:
        x[w * W:(w + 1) * W] = seg
    other, bg1, bg2 = (synth.noise_clips(1, W, seed=s)[0] for s in (43, 47, 53))
    bank = avex_amd.ExampleBank(768, class_names=["pasted", "other"])
    assert bank.add_clips(beats, [(x, 2.0, 3.0), other], [0, 1]) == range(0, 2)              # "the call is at 2.0-3.0 s of this recording"
    assert bank.add_clips(beats, [bg1, bg2], -1) == range(2, 4)
    assert len(bank) == 4 and bank.n_classes == 2 and bank.counts.tolist() == [1, 1, 2]
    kw = dict(layers=["last_layer"], batch_invariant=True, return_scores=True)
    first = avex_amd.detect_events_by_example(beats, bank, [x], 1.0, on=2.0, **kw)             # no cosine reaches 2: no event, but the scores
    assert int(first["count"]) == 0 and first["scores"].shape == (10, 2) and (first["row_of_window"].cpu().numpy() == np.arange(10)).all()
    s0 = first["scores"][:, 0].cpu().numpy()
    pasted, rest = s0[at], np.delete(s0, at)
    assert pasted.min() > rest.max(), (pasted, rest)
    assert abs(float(pasted.max()) - 1.0) < 1e-5
    on = np.array([0.5 * (float(pasted.min()) + float(rest.max())), 2.0], dtype=np.float32)
    res = avex_amd.detect_events_by_example(beats, bank, [x], 1.0, on=on, **kw)
    got = {k: v.cpu().numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}
    assert int(got["count"]) == 4 and got["class_id"].tolist() == [0] * 4 and got["recording"].tolist() == [0] * 4
    assert got["first"].tolist() == at == got["last"].tolist() == got["peak_window"].tolist()
    assert got["start_s"].tolist() == [float(w) for w in at] and got["end_s"].tolist() == [float(w + 1) for w in at]
    assert np.array_equal(_bits(got["scores"]), _bits(first["scores"].cpu().numpy()))
    hand = detection.detect_events(beats, bank.scorer(top_m=1, mode="similarity"), [x], 1.0, on=on, **kw)      # the scorer passed by hand
    for key, v in got.items():
        assert hand[key].cpu().numpy().tobytes() == v.tobytes(), key
    beats.deregister_all_hooks()

