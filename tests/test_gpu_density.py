"""Density clustering on the device: avex_amd.density over csrc/density.hip (avexhip_density_*).

1. inputs whose products are exact in fp32, eps exactly on an attained distance: every output equals the NumPy restatement
   (tests/_density_ref.py) bit for bit, across tile edges, both metrics, and at a size where a workgroup walks several column tiles;
2. random fp32 rows: the outputs equal the restatement applied to the device's own similarities, taken from an unmodified EmbeddingIndex
   over the same prepared rows -- the kernels run the shared tile, not a copy of it;
3. the recorded scikit-learn goldens, both metrics, every row;
4. a path of 1 025 points in shuffled row order, and two paths: the rounds end;
5. a border row within eps of core rows of two clusters takes the lower number, in both row orders;
6. the result does not depend on batch_size, chunk_rows, the pieces the rows were added in, or the run;
7. NaN, Inf and zero rows, min_samples above N, eps = 0 with duplicates;
8. sizes and exemplars, and the exemplars' metadata;
9. k_distance;
10. end to end: two call types pasted into noise recordings come out as two clusters, the background as noise.
"""
import os

import numpy as np
import pytest
import torch

import _density_ref as D
import avex_amd
from avex_amd import clustering, density, search, synth

pytestmark = pytest.mark.gpu

KEYS = ("labels", "core", "n_neighbors", "sizes", "exemplar")


def _host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _assert_same(got, want, what=""):
    got = _host(got)
    assert got["labels"].dtype == np.int32 and got["core"].dtype == np.bool_ and got["n_neighbors"].dtype == np.int32, what
    assert got["sizes"].dtype == np.int32 and got["exemplar"].dtype == np.int32, what
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())
    assert isinstance(got["n_clusters"], int) and got["n_clusters"] == want["n_clusters"] == len(got["sizes"]), what
    assert isinstance(got["nonfinite"], int) and got["nonfinite"] == want["nonfinite"], what
    assert isinstance(got["rounds"], int) and 1 <= got["rounds"] < 10000, what


def _same_bits(a, b, what=""):
    a, b = _host(a), _host(b)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape, (what, k)
    assert (a["n_clusters"], a["nonfinite"]) == (b["n_clusters"], b["nonfinite"]), what


def _pm1(name, n, d=16):
    return np.where(synth.normal(name, (n, d), 1.0) >= 0, 1.0, -1.0).astype(np.float32)


def _mirrored_ints(name, n, d=5):
    """Integers |x| <= 2, every row with its negative (and a zero row when n is odd): the column means are exactly 0 for n > 1."""
    a = np.clip(np.rint(synth.normal(name, (n // 2, d), 1.0)), -2, 2).astype(np.float32)
    return np.concatenate([a, -a] + ([np.zeros((1, d), dtype=np.float32)] if n % 2 else []))


def _device_sim(prepared_rows, metric):
    """The device's own similarities [n, n] of prepared rows, from an unmodified EmbeddingIndex ("dot": the rows are taken as they are)."""
    ix = search.EmbeddingIndex(int(prepared_rows.shape[1]), metric=metric, chunk_rows=4096)
    ix.add(prepared_rows)
    return ix.search(prepared_rows, 1, return_sim=True)["sim"].cpu().numpy()


def _centred_on_device(x):
    """X - mean as the centring pass of the clustering kernels leaves it: what dbscan(metric="euclidean") reads."""
    xd = torch.from_numpy(x).cuda()
    prep = clustering._Prepared(xd, 1, 1, 1e-4)
    ptr, ld = prep.centred_rows()
    off = ptr - prep.ws.data_ptr()
    return prep.ws[off:off + 4 * x.shape[0] * ld].view(torch.float32).view(x.shape[0], ld)[:, :x.shape[1]].clone()


# ------------------------------------------------------------------------------------------------------------------ 1. exact arithmetic
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257])
def test_exact_cosine_rows_equal_the_restatement(built_lib, n):
    """+-1 entries, d = 16: a prepared row is +-0.25, a similarity (16 - 2 h) / 16 and a distance h / 8 for Hamming distance h, all exact;
    eps = 0.375, 0.5 and 0.75 are attained distances, so the inclusive <= decides pairs."""
    x = _pm1(f"dens-pm1-{n}", n)
    sim = D.similarities(x, "cosine")
    assert np.array_equal(sim.astype(np.float64), D.prepared(x, "cosine").astype(np.float64) @ D.prepared(x, "cosine").astype(np.float64).T)
    at = mixed = 0
    for eps in (0.375, 0.5, 0.75):
        at += int((D.distances(sim, "cosine") == np.float32(eps)).sum())
        for ms in (1, 2, 5):
            want = D.dbscan(sim=sim, eps=eps, min_samples=ms, metric="cosine")
            _assert_same(density.dbscan(torch.from_numpy(x).cuda() if ms == 2 else x, eps, ms), want, f"eps={eps} ms={ms}")
            mixed += int(want["n_clusters"] >= 1 and (want["labels"] < 0).any() and (~want["core"] & (want["labels"] >= 0)).any())
    assert (at > 0 and mixed > 0) or n <= 2                                                 # pairs at the threshold; clusters, noise and border rows at once


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257])
def test_exact_euclidean_rows_equal_the_restatement(built_lib, n):
    """Small integers with column means exactly 0: centred rows, products, squared distances (integers) are exact, and the root of an
    integer is the correctly rounded one on both sides.  eps = sqrt(2) and 2 are attained distances."""
    x = _mirrored_ints(f"dens-int-{n}", n)
    assert x.shape[0] == n
    sim = D.similarities(x, "euclidean")
    p = D.prepared(x, "euclidean").astype(np.float64)
    assert np.array_equal(sim.astype(np.float64), p @ p.T) and (n == 1 or np.array_equal(p, x))
    at = 0
    for eps in (float(np.sqrt(np.float32(2.0))), 2.0):
        at += int((D.distances(sim, "euclidean") == np.float32(eps)).sum())
        for ms in (1, 2, 5):
            want = D.dbscan(sim=sim, eps=eps, min_samples=ms, metric="euclidean")
            _assert_same(density.dbscan(x, eps, ms, metric="euclidean"), want, f"eps={eps} ms={ms}")
    assert at > 0 or n <= 2


def test_segments_of_several_column_tiles(built_lib):
    """6 100 rows are 48 x 48 tiles: with one row block a workgroup walks two column tiles and carries its counts and minima from one to
    the next (2 048 workgroups at most per launch); with row blocks of 128 every workgroup has one tile.  Exact rows, as above."""
    n = 6100
    x = _pm1("dens-pm1-segments", n)
    want = D.dbscan(x, eps=0.25, min_samples=14, metric="cosine")
    assert want["n_clusters"] >= 1 and (want["labels"] < 0).any() and (~want["core"] & (want["labels"] >= 0)).any()
    got = density.dbscan(x, 0.25, 14)
    _assert_same(got, want)
    _same_bits(density.dbscan(x, 0.25, 14, batch_size=128), got, "one tile per workgroup")


# ------------------------------------------------------------------------------------------------------------------ 2. random rows
@pytest.mark.parametrize("metric", D.METRICS)
@pytest.mark.parametrize("d", [5, 33, 48])
def test_random_rows_equal_the_restatement_on_the_devices_similarities(built_lib, d, metric):
    n = 300
    x = D.planted(f"dens-rand-{d}", n, d)
    if metric == "cosine":
        sim = _device_sim(x, "cosine")                                                      # the index and the search prepare the rows by one code
    else:
        sim = _device_sim(_centred_on_device(x), "dot")
    assert np.array_equal(sim, sim.T)                                                       # s(i, j) and s(j, i) are the same bits
    dist = D.distances(sim, metric)
    for q in (0.03, 0.10):
        eps = float(np.quantile(dist[np.triu_indices(n, 1)], q))
        want = D.dbscan(sim=sim, eps=eps, min_samples=4, metric=metric)
        _assert_same(density.dbscan(x, eps, 4, metric=metric), want, f"q={q}")
    assert want["n_clusters"] >= 1 and want["nonfinite"] == 0


# ------------------------------------------------------------------------------------------------------------------ 3. scikit-learn goldens
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density.npz"))


@pytest.mark.parametrize("metric", D.METRICS)
@pytest.mark.parametrize("n,d", D.CASES, ids=[f"n{n}-d{d}" for n, d in D.CASES])
def test_equals_the_recorded_sklearn_dbscan(built_lib, golden, n, d, metric):
    key = f"{D.case_name(n, d)}/{metric}"
    x = D.planted(D.case_name(n, d), n, d)
    got = _host(density.dbscan(x, float(golden[f"{key}/eps"]), D.MIN_SAMPLES, metric=metric))
    assert np.array_equal(got["labels"], golden[f"{key}/labels"])
    assert np.array_equal(np.flatnonzero(got["core"]), golden[f"{key}/core"])
    assert got["n_clusters"] == int(golden[f"{key}/labels"].max()) + 1 and got["nonfinite"] == 0


# ------------------------------------------------------------------------------------------------------------------ 4. paths
def _path(n=1025, step=0.02, rise=3e-4):
    """n points at angle step `step` along a circle.  1 025 steps of 0.02 rad are 3.26 turns, and on a plain circle the turns would lie on
    top of each other; a third coordinate that rises by `rise` per point keeps them apart (one turn: cosine distance about 4e-3) and
    leaves the neighbours as on the arc: adjacent points at 1.8e-4 .. 2.0e-4, next-adjacent ones at 7.3e-4 .. 8.0e-4 (asserted in fp64)."""
    k = np.arange(n, dtype=np.float64)
    p = np.stack([np.cos(step * k), np.sin(step * k), rise * k], axis=1)
    u = p / np.linalg.norm(p, axis=1)[:, None]
    dist = 1.0 - u @ u.T
    band = np.abs(k[:, None] - k[None, :])
    assert dist[band == 1].max() < 2.01e-4 and dist[band >= 2].min() > 7.2e-4              # eps = 4e-4 is 2e-4 from either: 1 000 x the fp32 error
    return p.astype(np.float32)


def test_a_shuffled_path_is_one_cluster(built_lib):
    p = _path()
    order = np.random.RandomState(3).permutation(len(p))
    got = _host(density.dbscan(p[order], 4e-4, 3))
    print("path rounds", got["rounds"])
    assert got["n_clusters"] == 1 and 1 <= got["rounds"] < 10000 and got["sizes"].tolist() == [1025]
    where = np.argsort(order)                                                              # row of point k
    ends = where[[0, 1024]]
    assert (got["labels"] == 0).all() and not got["core"][ends].any() and got["core"].sum() == 1023
    assert got["n_neighbors"][ends].tolist() == [2, 2] and (np.delete(got["n_neighbors"], ends) == 3).all()
    _assert_same(got, D.dbscan(p[order], 4e-4, 3, "cosine"))
    with pytest.raises(avex_amd._capi.AvexHipError, match="max_rounds"):
        density.dbscan(p[order], 4e-4, 3, max_rounds=1)


def test_two_shuffled_paths_are_two_clusters_numbered_by_lowest_core_row(built_lib):
    p = np.delete(_path(), np.arange(500, 505), axis=0)                                     # a gap of six steps: cosine distance 7e-3
    order = np.random.RandomState(4).permutation(len(p))
    got = _host(density.dbscan(p[order], 4e-4, 3))
    where = np.argsort(order)
    first, second = where[:500], where[500:]
    assert got["n_clusters"] == 2 and sorted(got["sizes"].tolist()) == [500, 520] and 1 <= got["rounds"] < 10000
    a, b = np.unique(got["labels"][first]), np.unique(got["labels"][second])
    assert len(a) == len(b) == 1 and {int(a[0]), int(b[0])} == {0, 1}
    low = [int(np.flatnonzero(got["core"] & (got["labels"] == c)).min()) for c in (0, 1)]
    assert low[0] < low[1] and low[0] == int(np.flatnonzero(got["core"]).min())
    _assert_same(got, D.dbscan(p[order], 4e-4, 3, "cosine"))


# ------------------------------------------------------------------------------------------------------------------ 5. a shared border row
def test_a_border_row_between_two_clusters_takes_the_lower_number(built_lib):
    """Two plus signs around (0, 0) and (2, 0) that share the arm (1, 0); eps 1, min_samples 4: the centres alone are core."""
    x = np.array([[0, 0], [-1, 0], [0, 1], [0, -1], [1, 0], [2, 0], [3, 0], [2, 1], [2, -1]], dtype=np.float32)      # column means 1 and 0
    for rows, labels in ((x, [0, 0, 0, 0, 0, 1, 1, 1, 1]), (x[::-1].copy(), [0, 0, 0, 0, 0, 1, 1, 1, 1])):
        got = _host(density.dbscan(rows, 1.0, 4, metric="euclidean"))
        assert got["labels"].tolist() == labels and got["core"].sum() == 2 and got["sizes"].tolist() == [5, 4]
        assert got["n_neighbors"][4].item() == 3 and not got["core"][4]                     # the shared arm, in either order
        _assert_same(got, D.dbscan(rows, 1.0, 4, "euclidean"))


# ------------------------------------------------------------------------------------------------------------------ 6. independence
def test_the_result_does_not_depend_on_batches_chunks_pieces_or_the_run(built_lib):
    n, d = 300, 33
    x = D.planted(D.case_name(n, d), n, d)
    for metric in D.METRICS:
        eps, _ = D.gap_eps(x, metric)
        base = density.dbscan(x, eps, 4, metric=metric)
        assert base["n_clusters"] >= 2
        for batch_size in (128, 256, 4096):
            _same_bits(density.dbscan(x, eps, 4, metric=metric, batch_size=batch_size), base, f"{metric} batch {batch_size}")
        _same_bits(density.dbscan(x, eps, 4, metric=metric), base, f"{metric} again")
    eps, _ = D.gap_eps(x, "cosine")
    base = density.dbscan(x, eps, 4)
    for chunk_rows in (128, 256, 65536):
        ix = search.EmbeddingIndex(d, chunk_rows=chunk_rows)
        ix.add(x)
        _same_bits(density.dbscan(ix, eps, 4, batch_size=128 if chunk_rows == 256 else 65536), base, f"chunk_rows {chunk_rows}")
    ix = search.EmbeddingIndex(d, chunk_rows=128)
    for lo, hi in ((0, 100), (100, 101), (101, 300)):
        ix.add(torch.from_numpy(x[lo:hi]).cuda())
    _same_bits(density.dbscan(ix, eps, 4), base, "pieces")


# ------------------------------------------------------------------------------------------------------------------ 7. degenerate inputs
def test_nan_inf_and_zero_rows(built_lib):
    good = _pm1("dens-degenerate", 140)
    x = good.copy()
    bad = {5: np.nan, 64: np.inf, 127: -np.inf, 128: np.nan}
    for r, v in bad.items():
        x[r, r % 16] = v
    x[70] = 0.0
    got = _host(density.dbscan(x, 0.5, 5))
    _assert_same(got, D.dbscan(x, 0.5, 5, "cosine"))
    rows = sorted(bad)
    assert got["nonfinite"] == 4 and (got["n_neighbors"][rows] == 0).all() and (got["labels"][rows] == -1).all() and not got["core"][rows].any()
    assert got["n_neighbors"][70] == 1 and got["labels"][70] == -1                           # the zero row: at distance 1 from everything but itself
    keep = np.setdiff1d(np.arange(140), rows + [70])
    alone = _host(density.dbscan(good[keep], 0.5, 5))                                       # the others are what they are without them
    assert np.array_equal(alone["n_neighbors"], got["n_neighbors"][keep]) and np.array_equal(alone["core"], got["core"][keep])
    assert np.array_equal(alone["labels"], got["labels"][keep]) and alone["n_clusters"] == got["n_clusters"] >= 1
    every = _host(density.dbscan(np.full((3, 4), np.nan, dtype=np.float32), 0.5, 1))
    assert every["nonfinite"] == 3 and every["n_clusters"] == 0 and every["labels"].tolist() == [-1] * 3 and every["n_neighbors"].tolist() == [0] * 3


def test_min_samples_above_n_and_eps_zero_with_duplicates(built_lib):
    x = D.planted("dens-dup", 40, 33)
    none = _host(density.dbscan(x, 0.5, 41))
    assert none["n_clusters"] == 0 and (none["labels"] == -1).all() and not none["core"].any() and none["sizes"].shape == (0,) == none["exemplar"].shape
    assert (none["n_neighbors"] >= 1).all()
    for metric in D.METRICS:
        # cosine: +-1 rows, whose similarity to a copy is exactly 1; euclidean: any rows -- the norms are the diagonal of the same product
        base = _pm1("dens-dup-pm1", 30) if metric == "cosine" else x
        rows = np.concatenate([base[:30], base[:10], base[:5], base[3:4]])                  # rows 0 .. 4 three times (row 3 four times), 5 .. 9 twice
        mult = (rows[:, None, :] == rows[None, :, :]).all(axis=2).sum(axis=1)
        assert mult.tolist() == [3, 3, 3, 4, 3] + [2] * 5 + [1] * 20 + [3, 3, 3, 4, 3] + [2] * 5 + [3, 3, 3, 4, 3] + [4]
        got = _host(density.dbscan(rows, 0.0, 3, metric=metric))
        assert got["n_neighbors"].tolist() == mult.tolist(), metric                         # bit-identical rows are at distance exactly 0, no other pair is
        assert got["n_clusters"] == 5 and got["labels"][:5].tolist() == [0, 1, 2, 3, 4] and (got["labels"][5:30] == -1).all(), metric
        assert got["sizes"].tolist() == [3, 3, 3, 4, 3] and got["exemplar"].tolist() == [0, 1, 2, 3, 4], metric


# ------------------------------------------------------------------------------------------------------------------ 8. sizes, exemplars
def test_sizes_exemplars_and_their_metadata(built_lib):
    n, d = 384, 48
    x = D.planted(D.case_name(n, d), n, d)
    eps, _ = D.gap_eps(x, "cosine")
    rec = (np.arange(n) // 100).astype(np.int32)
    start = (np.arange(n) % 100) * 0.5
    ix = search.EmbeddingIndex(d, chunk_rows=256)
    ix.add(x, recording=rec, start_s=start, end_s=start + 1.0)
    got = _host(density.dbscan(ix, eps, D.MIN_SAMPLES))
    sim = ix.search_rows(np.arange(n), 1, exclude=None, return_sim=True)["sim"].cpu().numpy()
    want = D.dbscan(sim=sim, eps=eps, min_samples=D.MIN_SAMPLES, metric="cosine")
    _assert_same(got, want)
    assert got["n_clusters"] >= 3 and got["sizes"].sum() == (got["labels"] >= 0).sum()
    for c, e in enumerate(got["exemplar"]):
        members = np.flatnonzero(got["core"] & (got["labels"] == c))
        assert e in members and got["n_neighbors"][e] == got["n_neighbors"][members].max() and e == members[got["n_neighbors"][members] == got["n_neighbors"][e]].min()
    e = got["exemplar"]
    assert got["exemplar_recording"].tolist() == rec[e].tolist() and got["exemplar_start_s"].tolist() == start[e].tolist()
    assert got["exemplar_end_s"].tolist() == (start[e] + 1.0).tolist()
    assert "exemplar_recording" not in density.dbscan(x, eps, D.MIN_SAMPLES)                # rows without an index carry no metadata


# ------------------------------------------------------------------------------------------------------------------ 9. k_distance
@pytest.mark.parametrize("n", [2, 127, 129, 257])
def test_k_distance_on_exact_rows(built_lib, n):
    x = _pm1(f"dens-pm1-{n}", n)
    sim = D.similarities(x, "cosine")
    ix = search.EmbeddingIndex(16, chunk_rows=128)
    ix.add(x)
    for k in (1, 5):
        got = density.k_distance(ix, k)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (n,)
        want = D.k_distance(sim, k)
        assert np.array_equal(got.cpu().numpy(), want), k
        if n > k:                                                                           # k here is min_samples = k + 1 there
            core = density.dbscan(ix, 0.5, k + 1)["core"].cpu().numpy()
            assert np.array_equal(core, want <= np.float32(0.5))


# ------------------------------------------------------------------------------------------------------------------ 10. end to end
@pytest.fixture(scope="module")
def beats(built_lib):
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=2)
    m = avex_amd.beats_model.Model(device="cuda", init_config=cfg, return_features_only=True, batch_invariant=True).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.beats_state_dict(cfg, seed=0).items()}, strict=False)
    return m


def test_two_pasted_call_types_come_out_as_two_clusters(beats):
    W = 16000
    recs = [synth.noise_clips(1, 10 * W, seed=s)[0].copy() for s in (61, 67)]
    calls = [synth.noise_clips(1, W, seed=s)[0] for s in (71, 73)]
    at = {0: [(0, 1), (0, 4), (1, 2), (1, 8)], 1: [(0, 6), (0, 8), (1, 0), (1, 5)]}          # call type -> (recording, second) it is pasted at
    for c, places in at.items():
        for r, w in places:
            recs[r][w * W:(w + 1) * W] = calls[c]
    ix = avex_amd.EmbeddingIndex.from_recordings(beats, recs, 1.0, layers=["last_layer"], batch_invariant=True, names=["a", "b"])
    beats.deregister_all_hooks()
    assert len(ix) == 20
    rows = {c: [10 * r + w for r, w in places] for c, places in at.items()}
    sim = ix.search_rows(np.arange(20), 1, exclude=None, return_sim=True)["sim"].cpu().numpy()
    dist = D.distances(sim, "cosine")
    same = np.zeros((20, 20), dtype=bool)
    for c in rows:
        same[np.ix_(rows[c], rows[c])] = True
    off = ~same & ~np.eye(20, dtype=bool)
    print("within a call type <=", dist[same].max(), "every other pair >=", dist[off].min())
    assert dist[same].max() < 1e-5 and dist[off].min() > 4 * max(float(dist[same].max()), 1e-6)      # identical audio: distance 0 up to rounding
    eps = 0.5 * (float(dist[same].max()) + float(dist[off].min()))
    got = _host(avex_amd.dbscan(ix, eps, 3))
    assert got["n_clusters"] == 2 and got["sizes"].tolist() == [4, 4] and got["nonfinite"] == 0
    first = 0 if min(rows[0]) < min(rows[1]) else 1
    assert (got["labels"][rows[first]] == 0).all() and (got["labels"][rows[1 - first]] == 1).all()
    background = np.setdiff1d(np.arange(20), rows[0] + rows[1])
    assert (got["labels"][background] == -1).all() and (got["n_neighbors"][background] == 1).all()
    for c, e in enumerate(got["exemplar"]):                                                 # an exemplar's span is a span its call was pasted at
        r, w = int(got["exemplar_recording"][c]), got["exemplar_start_s"][c]
        assert (r, int(w)) in at[first if c == 0 else 1 - first] and got["exemplar_end_s"][c] == w + 1.0
    kd = avex_amd.k_distance(ix, 2).cpu().numpy()                                           # the curve eps is read from: a step between the calls and the rest
    assert kd[rows[0] + rows[1]].max() < eps < kd[background].min()
