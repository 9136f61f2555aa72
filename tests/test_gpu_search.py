"""Query-by-example search on the device: avex_amd.search over csrc/search.hip (avexhip_search_*).

1. inputs whose products are exact in fp32: similarities, scores, rows and counts equal the NumPy restatement (tests/_search_ref.py) bit for
   bit, ties included, across chunk, tile and batch edges and every k up to 1 024;
2. random fp32 rows: the selection is exact on the device's own similarities, which are within 4 x NumPy's fp32 error of fp64;
3. results do not depend on chunk_rows, batch_size, the pieces the rows were added in, or the run;
4. a list of 1 024 survives 18 merges;
5. NaN and zero rows, the query's own row, both exclusion modes and the suppression against the restatement; NaN spans; the split
   stages of the benchmark give the bits of the fused call;
6. end to end: a segment pasted into a recording is found where it was pasted;
7. an index that went through state_dict answers with the same bits.
"""
import io

import numpy as np
import pytest
import torch

import _search_ref as S
import avex_amd
from avex_amd import search, synth

pytestmark = pytest.mark.gpu

KEYS = ("scores", "rows", "count", "recording", "start_s", "end_s")


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _assert_same(got, want, what=""):
    """Integer for integer and bit for bit (NaN spans past `count` compare as their bits too)."""
    for key in KEYS:
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype.kind == "f":
            gi, wi = g.view(f"i{g.itemsize}"), w.view(f"i{w.itemsize}")
            nan = np.isnan(g) & np.isnan(w)                              # any NaN is "no span": payload bits are not part of the contract
            assert np.array_equal(gi[~nan], wi[~nan]), (what, key, np.argwhere((gi != wi) & ~nan)[:5])
        else:
            assert np.array_equal(g, w), (what, key, np.argwhere(g != w)[:5])


def _pm1(name, shape):
    return np.where(synth.normal(name, shape, 1.0) >= 0, 1.0, -1.0).astype(np.float32)


def _small_ints(name, shape):
    return np.clip(np.rint(synth.normal(name, shape, 1.5)), -3, 3).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ 1. exact order
ALL_K = (1, 2, 31, 32, 33, 64, 1000, 1024)
#         metric    d   rows  chunk_rows  nq  batch_size  ks
EXACT = [("cosine", 16, 1, 128, 1, 1, ALL_K),
         ("cosine", 64, 127, 128, 127, 128, ALL_K),
         ("cosine", 256, 128, 128, 129, 128, ALL_K),
         ("cosine", 16, 129, 128, 300, 1024, ALL_K),
         ("dot", 1, 255, 256, 1, 1, ALL_K),
         ("dot", 33, 256, 256, 127, 1, ALL_K),
         ("dot", 100, 257, 256, 129, 128, ALL_K),
         ("dot", 768, 1000, 128, 300, 1024, ALL_K),
         ("cosine", 64, 1000, 256, 300, 1, (1, 33, 1000, 1024)),
         ("dot", 33, 1000, 128, 129, 128, ALL_K),
         ("cosine", 256, 255, 256, 127, 1024, ALL_K),
         ("dot", 100, 1000, 256, 1, 1, ALL_K)]


@pytest.mark.parametrize("metric,d,rows,chunk_rows,nq,batch_size,ks", EXACT, ids=[f"{c[0]}-d{c[1]}-n{c[2]}-c{c[3]}-q{c[4]}-b{c[5]}" for c in EXACT])
def test_exact_arithmetic_exact_order(built_lib, metric, d, rows, chunk_rows, nq, batch_size, ks):
    """+-1 entries with d in {16, 64, 256} (norms 4, 8, 16) and integers |x| <= 3: every product and partial sum is exact in fp32, so the
    similarities, and with them the order, ties included, are known without a tolerance."""
    make = _pm1 if metric == "cosine" else _small_ints
    db, q = make(f"srch-db-{d}-{rows}", (rows, d)), make(f"srch-q-{d}-{nq}", (nq, d))
    want_sim = S.prepared(q, metric) @ S.prepared(db, metric).T
    assert np.array_equal(want_sim.astype(np.float64), S.prepared(q, metric).astype(np.float64) @ S.prepared(db, metric).astype(np.float64).T)      # exact indeed
    ix = search.EmbeddingIndex(d, metric=metric, chunk_rows=chunk_rows)
    assert ix.add(db) == range(0, rows) and len(ix) == rows
    if rows > 1:
        assert int((np.diff(np.sort(want_sim, axis=1), axis=1) == 0).sum()) > 0      # there are ties to break
    for k in ks:
        got = _host(ix.search(q, k, batch_size=batch_size, return_sim=(k == ks[0])))
        if k == ks[0]:
            assert np.array_equal(got["sim"], want_sim)
        _assert_same(got, S.search(want_sim, k), f"k={k}")
        assert (got["count"] == min(k, rows)).all()


# ------------------------------------------------------------------------------------------------------------------ 2. random rows
def _device_prepared(x, metric):
    """Rows as the device prepares them (the restatement sums a norm's squares in another order)."""
    ix = search.EmbeddingIndex(x.shape[1], metric=metric, chunk_rows=4096)
    ix.add(x)
    return ix.state_dict()["rows"]


@pytest.mark.parametrize("metric,d", [("cosine", 768), ("dot", 40), ("cosine", 40)])
def test_random_rows_selection_and_similarity_error(built_lib, metric, d):
    db = synth.normal(f"srch-rand-db-{d}", (5000, d), 1.0).astype(np.float32)
    q = synth.normal(f"srch-rand-q-{d}", (200, d), 1.0).astype(np.float32)
    ix = search.EmbeddingIndex(d, metric=metric, chunk_rows=2048)
    ix.add(torch.from_numpy(db).cuda())
    got = _host(ix.search(torch.from_numpy(q).cuda(), 50, batch_size=128, return_sim=True))
    sim = got["sim"]
    assert sim.shape == (200, 5000) and sim.dtype == np.float32 and np.isfinite(sim).all()
    _assert_same(got, S.search(sim, 50), metric)                                               # exact on the device's OWN similarities, every query
    assert np.array_equal(got["scores"].view(np.int32), np.take_along_axis(sim, got["rows"], axis=1).view(np.int32))
    pd, pq = _device_prepared(db, metric), _device_prepared(q, metric)
    assert np.array_equal(pd, ix.state_dict()["rows"])
    if metric == "cosine":
        # entries <= 1; the two sums of d <= 768 squares err by at most (12 + 6) and 10 roundings of 2^-24 relative, the root halves that
        assert np.abs(pd - S.prepared(db, metric)).max() <= 2.0 ** -20
    else:
        assert np.array_equal(pd, db)
    ref64 = pq.astype(np.float64) @ pd.astype(np.float64).T
    err_np = float(np.abs((pq @ pd.T).astype(np.float64) - ref64).max())
    err = float(np.abs(sim.astype(np.float64) - ref64).max())
    print(f"[search] {metric} d={d}: similarity max abs error {err:.3e} (NumPy fp32 {err_np:.3e})")
    assert err <= 4.0 * err_np, (err, err_np)


# ------------------------------------------------------------------------------------------------------------------ 3. invariance
def test_results_do_not_depend_on_chunks_batches_pieces_or_the_run(built_lib):
    d, n, nq, k = 40, 1000, 130, 33
    db = synth.normal("srch-inv-db", (n, d), 1.0).astype(np.float32)
    db[500:520] = db[100:120]                                                                   # twenty exact ties per query, 400 rows apart
    q = synth.normal("srch-inv-q", (nq, d), 1.0).astype(np.float32)
    rec = (np.arange(n) // 100).astype(np.int32)
    start = (np.arange(n) % 100) * 0.25
    base = None
    for chunk_rows, batch_size, pieces in ((128, 1024, None), (256, 100, None), (4096, 1, None), (128, 100, (1, 130, 7, 256, 606)), (256, 1024, (999, 1)),
                                           (128, 1024, None)):
        ix = search.EmbeddingIndex(d, chunk_rows=chunk_rows)
        lo = 0
        for p in pieces or (n,):
            assert ix.add(db[lo:lo + p], recording=rec[lo:lo + p], start_s=start[lo:lo + p], end_s=start[lo:lo + p] + 1.0) == range(lo, lo + p)
            lo += p
        assert lo == n == len(ix)
        runs = [_host(ix.search(q, k, batch_size=batch_size, return_sim=True)), _host(ix.search(q, k, nms=0.5, batch_size=batch_size))]
        runs.append(_host(ix.search(q, k, batch_size=batch_size, return_sim=True)))            # a second run
        assert np.array_equal(runs[0]["sim"].view(np.int32), runs[2]["sim"].view(np.int32))
        _assert_same(runs[0], runs[2], "second run")
        if base is None:
            base = runs
            _assert_same(runs[0], S.search(runs[0]["sim"], k, rec=rec, start=start, end=start + 1.0), "base")
            _assert_same(runs[1], S.search(runs[0]["sim"], k, nms_overlap=0.5, rec=rec, start=start, end=start + 1.0), "base nms")
            ties = (runs[0]["sim"][:, 100:120] == runs[0]["sim"][:, 500:520])
            assert ties.all()                                                                   # a similarity depends on its two rows only
            continue
        what = f"chunk_rows={chunk_rows} batch_size={batch_size} pieces={pieces}"
        assert np.array_equal(runs[0]["sim"].view(np.int32), base[0]["sim"].view(np.int32)), what
        _assert_same(runs[0], base[0], what)
        _assert_same(runs[1], base[1], what + " nms")


# ------------------------------------------------------------------------------------------------------------------ 4. deep list
def test_a_list_of_1024_survives_18_merges(built_lib):
    n, d, nq, k = 70000, 32, 64, 1024
    db, q = _small_ints("srch-deep-db", (n, d)), _small_ints("srch-deep-q", (nq, d))
    ix = search.EmbeddingIndex(d, metric="dot", chunk_rows=4096)
    ix.add(db[:30000])
    ix.add(torch.from_numpy(db[30000:]).cuda())
    assert len(ix._chunks) == 18 and len(ix) == n
    got = _host(ix.search(q, k, return_sim=True))
    assert np.array_equal(got["sim"], q @ db.T)                                                 # integers: exact
    want = S.search(got["sim"], k)
    _assert_same(got, want, "deep")
    assert (got["count"] == k).all() and int((got["rows"] >= 65536).sum()) > 0 and int((got["rows"] < 4096).sum()) > 0
    assert (np.diff(got["scores"], axis=1) <= 0).all() and int((np.diff(got["scores"], axis=1) == 0).sum()) > nq * 500      # long runs of ties, in row order


# ------------------------------------------------------------------------------------------------------------------ 5. filters
N_REC, N_WIN = 6, 40


def _recordings_index(n_rec=N_REC, chunk_rows=128, d=32, extra=True):
    """n_rec synthetic recordings of 40 windows of 1 s with hop 0.25 s (spans are multiples of 0.25: exact in fp64), then a NaN row and an
    all-zero row without metadata."""
    x = synth.normal(f"srch-filt-{n_rec}", (n_rec * N_WIN, d), 1.0).astype(np.float32)
    x += 2.0 * np.repeat(synth.normal(f"srch-filt-c-{n_rec}", (n_rec, d), 1.0).astype(np.float32), N_WIN, axis=0)      # windows of a recording resemble each other
    rec = np.repeat(np.arange(n_rec, dtype=np.int32), N_WIN)
    start = np.tile(np.arange(N_WIN) * 0.25, n_rec)
    ix = search.EmbeddingIndex(d, chunk_rows=chunk_rows)
    for r in range(n_rec):
        s = slice(r * N_WIN, (r + 1) * N_WIN)
        assert ix.add_recording({"embeddings": torch.from_numpy(x[s]).cuda(), "start_s": start[s], "end_s": start[s] + 1.0}, name=f"rec{r}") == r
    if extra:
        tail = np.zeros((2, d), dtype=np.float32)
        tail[0, 3] = np.nan
        ix.add(tail)
        rec = np.concatenate([rec, np.array([-1, -1], dtype=np.int32)])
        start = np.concatenate([start, [np.nan, np.nan]])
    return ix, rec, start, start + 1.0


def test_filters_against_the_restatement(built_lib):
    ix, rec, start, end = _recordings_index()
    n = len(ix)
    assert n == 242 and ix.n_recordings == 6 and ix.names == [f"rec{r}" for r in range(6)]
    rows = np.arange(n)
    full = _host(ix.search_rows(rows, 10, exclude=None, return_sim=True))
    sim = full["sim"]
    assert np.isnan(sim[:, 240]).all() and np.isnan(sim[240]).all() and (sim[:240, 241] == 0).all()      # the NaN row is never a hit; the zero row scores 0
    assert not (full["rows"] == 240).any() and not (full["rows"] == rows[:, None]).any()        # nor is the query's own row
    assert full["count"][240] == 0 and (full["rows"][240] == -1).all() and np.isneginf(full["scores"][240]).all()
    _assert_same(full, S.search(sim, 10, skip_rows=rows, rec=rec, start=start, end=end), "skip")
    masks = {mode: np.stack([S.exclude_mask(mode, rec[r], start[r], end[r], rec, start, end) for r in rows]) for mode in ("recording", "overlap")}
    assert masks["overlap"][5].sum() == 7 and masks["recording"][5].sum() == 40 and masks["overlap"][241].sum() == 0
    for mode in ("recording", "overlap"):
        for nms in (None, 0.0, 0.5):
            got = _host(ix.search_rows(torch.from_numpy(rows).cuda(), 10, exclude=mode, nms=nms, batch_size=100))
            _assert_same(got, S.search(sim, 10, nms_overlap=nms, skip_rows=rows, excluded=masks[mode], rec=rec, start=start, end=end), f"{mode} nms={nms}")
            hit_rec = np.where(got["rows"] >= 0, rec[got["rows"]], -2)
            if mode == "recording":
                assert not (hit_rec[:240] == rec[:240, None]).any()
    default = _host(ix.search_rows(rows, 10))                                                   # exclude defaults to "overlap"
    _assert_same(default, S.search(sim, 10, skip_rows=rows, excluded=masks["overlap"], rec=rec, start=start, end=end), "default")
    # search() with the metadata handed in: the same rows as queries, read back from the index
    q = torch.from_numpy(ix.state_dict()["rows"][:240]).cuda()
    ext = _host(ix.search(q, 10, exclude="overlap", nms=0.0, query_recording=rec[:240], query_start_s=start[:240], query_end_s=end[:240], return_sim=True))
    _assert_same(ext, S.search(ext["sim"], 10, nms_overlap=0.0, excluded=masks["overlap"][:240], rec=rec, start=start, end=end), "search + metadata")
    one = _host(ix.search(q[:3], 5, exclude="recording", query_recording="rec0"))              # one recording, by name, for all queries
    assert not (rec[one["rows"]] == 0).any() and (one["count"] == 5).all()
    # suppression leaves fewer than k: at most ten windows of a recording are disjoint, and the two rows without metadata always survive
    few = _host(ix.search(q[:20], 200, nms=0.0, return_sim=True))
    _assert_same(few, S.search(few["sim"], 200, nms_overlap=0.0, rec=rec, start=start, end=end), "fewer than k")
    assert (few["count"] < 200).all() and (few["count"] >= 7).all() and (few["count"] <= 61).all()
    assert (few["rows"][np.arange(20), few["count"] - 1] >= 0).all() and (few["rows"][np.arange(20), few["count"]] == -1).all()
    for b in range(20):                                                                         # what survives is disjoint within a recording
        r = few["rows"][b, :few["count"][b]]
        for rr in range(N_REC):
            s = np.sort(start[r[rec[r] == rr]])
            assert (np.diff(s) >= 1.0).all()


def test_overfetch_is_capped_at_1024_candidates(built_lib):
    ix, rec, start, end = _recordings_index(n_rec=30, chunk_rows=256, extra=False)
    assert len(ix) == 1200
    q = torch.from_numpy(synth.normal("srch-cap-q", (16, 32), 1.0).astype(np.float32)).cuda()
    got = _host(ix.search(q, 300, nms=0.0, overfetch=4, return_sim=True))                       # K' = min(1200, 1024)
    capped = S.search(got["sim"], 300, nms_overlap=0.0, overfetch=4, rec=rec, start=start, end=end)
    _assert_same(got, capped, "capped")
    uncapped = S.search(got["sim"], 300, nms_overlap=0.0, overfetch=4, rec=rec, start=start, end=end, max_k=1 << 20)
    assert (uncapped["count"] >= capped["count"]).all() and (uncapped["count"] > capped["count"]).any()      # the cap is what was compared
    three = _host(ix.search(q, 300, nms=0.0, overfetch=3))                                      # K' = 900: under the cap
    _assert_same(three, S.search(got["sim"], 300, nms_overlap=0.0, overfetch=3, rec=rec, start=start, end=end), "overfetch 3")


def test_nan_spans_in_a_recording_with_spans(built_lib):
    """One recording mixes rows with and without spans (added with the id alone).  NumPy's minimum / maximum carry the NaN and every
    compare with it is false, so such a row is not excluded by "overlap", excludes nothing as a query, and neither suppresses nor is
    suppressed; the device must do the same."""
    d, n = 32, 300
    x = synth.normal("srch-nanspan", (n, d), 1.0).astype(np.float32) + 2.0 * synth.normal("srch-nanspan-c", (1, d), 1.0).astype(np.float32)
    rec = (np.arange(n) // 150).astype(np.int32)                                                 # two recordings of 150 rows
    start = (np.arange(n) % 150) * 0.25
    bare = (np.arange(n) % 3) == 1                                                               # every third row has no span
    start[bare] = np.nan
    ix = search.EmbeddingIndex(d, chunk_rows=128)
    ix.add(x[:150][~bare[:150]], recording=0, start_s=start[:150][~bare[:150]], end_s=start[:150][~bare[:150]] + 1.0)
    ix.add(x[:150][bare[:150]], recording=0)
    ix.add(torch.from_numpy(x[150:]).cuda(), recording=rec[150:], start_s=torch.from_numpy(start[150:]).cuda(), end_s=torch.from_numpy(start[150:] + 1.0).cuda())
    assert len(ix) == n
    assert ix.names == ["0", "1"] and ix.n_recordings == 2                                       # ids given on the host are registered
    order = np.concatenate([np.flatnonzero(~bare[:150]), np.flatnonzero(bare[:150]), np.arange(150, n)])
    rec, start = rec[order], start[order]
    end = start + 1.0
    st = ix.state_dict()
    assert np.array_equal(st["recording"], rec) and np.array_equal(np.isnan(st["start_s"]), np.isnan(start)) and int(np.isnan(start).sum()) == 100
    rows = np.arange(n)
    sim = _host(ix.search_rows(rows, 5, exclude=None, return_sim=True))["sim"]
    mask = np.stack([S.exclude_mask("overlap", rec[r], start[r], end[r], rec, start, end) for r in rows])
    assert not mask[np.isnan(start)].any() and not mask[:, np.isnan(start)].any() and mask.any()
    for nms in (None, 0.0, 0.5):
        got = _host(ix.search_rows(rows, 40, nms=nms, batch_size=128))                           # exclude="overlap"
        want = S.search(sim, 40, nms_overlap=nms, skip_rows=rows, excluded=mask, rec=rec, start=start, end=end)
        _assert_same(got, want, f"nan spans nms={nms}")
        if nms is not None:                                                                      # rows without spans sit among the kept hits
            assert int(np.isnan(got["start_s"][:, :5]).sum()) > 0 and (got["count"] > 0).all()


def test_split_stages_give_the_bits_of_the_fused_call(built_lib):
    """`_timing` (scripts/search_bench.py) launches every chunk's similarity and select stage on their own (`stages` 1, then 2, of
    avexhip_search_chunk) with events between them: the same results, and three device times."""
    ix, rec, start, end = _recordings_index(n_rec=30, chunk_rows=256, extra=False)               # 1 200 rows: five chunks
    q = torch.from_numpy(synth.normal("srch-split-q", (130, 32), 1.0).astype(np.float32)).cuda()
    for kw in (dict(k=10), dict(k=300, nms=0.5), dict(k=1024), dict(k=7, nms=0.0, exclude="recording", query_recording=3)):
        fused = _host(ix.search(q, batch_size=100, return_sim=True, **kw))
        timing = {}
        split = _host(ix.search(q, batch_size=100, return_sim=True, _timing=timing, **kw))
        assert np.array_equal(fused["sim"].view(np.int32), split["sim"].view(np.int32)), kw
        _assert_same(split, fused, str(kw))
        _assert_same(fused, S.search(fused["sim"], kw["k"], nms_overlap=kw.get("nms"), rec=rec, start=start, end=end,
                                     excluded=None if "exclude" not in kw else np.tile(rec == 3, (130, 1))), str(kw))
        assert sorted(timing) == ["finish_s", "select_s", "similarity_s"] and all(v > 0.0 for v in timing.values()), timing


# ------------------------------------------------------------------------------------------------------------------ 6. end to end
@pytest.fixture(scope="module")
def beats(built_lib):
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=2)
    m = avex_amd.beats_model.Model(device="cuda", init_config=cfg, return_features_only=True, batch_invariant=True).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.beats_state_dict(cfg, seed=0).items()}, strict=False)
    return m


def test_a_pasted_segment_is_found_where_it_was_pasted(beats):
    sr, W = 16000, 16000
    x = synth.noise_clips(1, 10 * W, seed=31)[0].copy()
    y = synth.noise_clips(1, 4 * W, seed=37)[0]
    seg = synth.noise_clips(1, W, seed=41)[0]
    at = [2, 4, 7, 9]
    for w in at:
        x[w * W:(w + 1) * W] = seg
    ix = avex_amd.EmbeddingIndex.from_recordings(beats, [y, x], 1.0, layers=["last_layer"], batch_invariant=True, chunk_rows=128, names=["other", "pasted"])
    assert len(ix) == 14 and ix.dim == 768 and ix.names == ["other", "pasted"] and ix.n_recordings == 2
    want = [4 + w for w in at]                                                                   # the first recording holds rows 0 .. 3
    got = _host(avex_amd.query_by_example(beats, ix, seg, k=6))
    assert got["rows"][0, :4].tolist() == want and got["count"].tolist() == [6]
    s = got["scores"][0]
    assert s[0] == s[1] == s[2] == s[3] and s[3] > s[4] and abs(float(s[0]) - 1.0) < 1e-5       # identical inputs, bit-identical embeddings
    assert got["recording"][0, :4].tolist() == [1] * 4 and got["start_s"][0, :4].tolist() == [float(w) for w in at]
    assert got["end_s"][0, :4].tolist() == [float(w + 1) for w in at]
    mine = _host(ix.search_rows([want[0]], 5))                                                   # exclude="overlap": its own window goes, the other three lead
    assert mine["rows"][0, :3].tolist() == want[1:] and mine["scores"][0, 0] == mine["scores"][0, 2] > mine["scores"][0, 3]
    assert want[0] not in mine["rows"][0].tolist()


# ------------------------------------------------------------------------------------------------------------------ 7. state
def test_state_dict_round_trip_gives_the_same_bits(built_lib):
    ix, rec, start, end = _recordings_index()
    q = torch.from_numpy(synth.normal("srch-state-q", (70, 32), 1.0).astype(np.float32)).cuda()
    buf = io.BytesIO()
    np.savez(buf, **ix.state_dict())
    buf.seek(0)
    back = search.EmbeddingIndex.from_state_dict(dict(np.load(buf)))
    assert len(back) == len(ix) and back.names == ix.names and back.metric == ix.metric and back.chunk_rows == ix.chunk_rows
    st0, st1 = ix.state_dict(), back.state_dict()
    for key in st0:
        a, b = st0[key], st1[key]
        assert a.dtype == b.dtype and a.shape == b.shape and (a.tobytes() == b.tobytes()), key
    for kw in (dict(k=10), dict(k=20, nms=0.5), dict(k=5, exclude="overlap", query_recording=2, query_start_s=3.0, query_end_s=4.0)):
        a, b = _host(ix.search(q, return_sim=True, **kw)), _host(back.search(q, return_sim=True, **kw))
        assert np.array_equal(a["sim"].view(np.int32), b["sim"].view(np.int32))
        _assert_same(a, b, str(kw))
    rows = [0, 57, 239]
    _assert_same(_host(ix.search_rows(rows, 8, nms=0.0)), _host(back.search_rows(rows, 8, nms=0.0)), "search_rows")
