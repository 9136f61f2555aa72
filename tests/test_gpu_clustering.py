"""avex_amd.clustering on the device against the real reference's outputs (tests/golden/clustering.npz, made by
tests/golden/make_clustering_goldens.py from avex/evaluation/clustering.py and scikit-learn) and, stage by stage, against the NumPy
restatement (tests/_clustering_ref.py).  Nothing here reads the reference tree or needs scikit-learn.

The contract is the reference's PARTITION, not scores within a tolerance: k-means is seeded, the goldens are sets whose partition
survives input noise of 1e-6 and whose runner-up partitions are at least 1e-5 (relative) away in inertia, and the three scores are
functions of the contingency table alone -- so they must then agree to fp64 rounding (1e-12)."""
import numpy as np
import pytest
import torch

import _clustering_ref as CR

pytestmark = pytest.mark.gpu

KEYS = ("clustering_ari", "clustering_nmi", "clustering_v_measure")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return CR.load_golden(golden_dir)


@pytest.fixture(scope="module")
def wide(golden_dir):
    return CR.load_wide(golden_dir)


WIDE = ("wide8_d1280", "wide10_d1536", "set40_k150", "set20_k200")      # the clustering cases of tests/golden/metrics_wide.npz


@pytest.fixture(scope="module")
def K(built_lib):
    from avex_amd import clustering
    return clustering


def _np(t):
    return t.cpu().numpy()


def _check_cases_reproduce_the_reference(K, z, meta, names):
    assert meta["max_unstable"] == 0
    for name in names:
        c = meta["cases"][name]
        x, lab = CR.case_inputs(z, meta, name)
        got = K.eval_clustering(x, lab, n_clusters=c["n_clusters"])
        ref = c["eval_clustering"]
        print(f"[clustering] {name}: device {got} reference {ref}")
        assert set(got) == set(KEYS)
        if f"{name}/km_labels" in z:
            km = K.kmeans(x, c["k"])
            same = CR.same_partition(_np(km["labels"]), z[f"{name}/km_labels"])
            print(f"[clustering] {name}: same partition {same}, n_iter {km['n_iter']} (reference {c['n_iter']}), best_init {km['best_init']}, "
                  f"inertia {km['inertia']!r} (reference {c['inertia']!r})")
            assert same, name
            assert km["n_iter"] == c["n_iter"], name
        for key in KEYS:
            assert abs(got[key] - ref[key]) <= 1e-12, (name, key, got[key], ref[key])


def test_every_golden_case_reproduces_the_reference(K, golden):
    """eval_clustering on every golden case: the reference's three scores within 1e-12, and (through kmeans) its partition."""
    z, meta = golden
    _check_cases_reproduce_the_reference(K, z, meta, list(meta["cases"]))


@pytest.mark.parametrize("name", WIDE)
def test_every_wide_case_reproduces_the_reference(K, wide, name):
    """The same contract past the shapes of clustering.npz.  dpad = 1280 / 1536 > 1024: the second column block of clus_update_kernel
    (blockIdx.y = 1) and the second trip of the col += 1024 loops of clus_seed_pick_kernel / clus_relocate_kernel and of the e += 1024
    loop of clus_decide_kernel past one row.  k = 150 / 200 (kpad 160 / 224): a restart's centres span two 128-column tiles of
    clus_assign_kernel and meet only in the 64-bit atomicMin, restart and tile boundaries fall at different columns, trials_of(k) = 7,
    and clus_seed_dist_kernel sees 70 candidates (more than 64)."""
    z, meta = wide
    assert set(meta["cases"]) == set(WIDE)
    _check_cases_reproduce_the_reference(K, z, meta, [name])


def test_multiple_k_matches_the_reference(K, golden):
    z, meta = golden
    mk = meta["multiple_k"]
    x, lab = CR.case_inputs(z, meta, mk["case"])
    got = K.eval_clustering_multiple_k(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda())
    print(f"[clustering] multiple_k: device {got} reference {mk['result']}")
    assert set(got) == set(mk["result"])
    for key, v in mk["result"].items():
        assert abs(got[key] - v) <= 1e-12, (key, got[key], v)
    for k, c in mk["per_k"].items():
        one = K.eval_clustering(x, lab, n_clusters=int(k))
        for key in KEYS:
            assert abs(one[key] - c["eval_clustering"][key]) <= 1e-12, (k, key)


def test_seeding_matches_the_restatement_and_the_reference(K, golden):
    """k-means++ stage: the seed rows of EVERY restart against the restatement (same draws, same summation order: equal), and the first
    restart's against sklearn.cluster.kmeans_plusplus as recorded in the golden."""
    z, meta = golden
    _check_seeding(K, z, meta, ("set8", "set30_d100", "set12_k30", "label_minus1", "n6_k10"))


@pytest.mark.parametrize("name", WIDE)
def test_seeding_of_the_wide_cases_matches_the_restatement_and_the_reference(K, wide, name):
    """clus_seed_dist_kernel / clus_seed_pick_kernel at dpad > 1024 (the chosen row is copied into the centre table in two trips) and with
    7 trials x 10 restarts = 70 candidates per step (five candidate groups of 16): all ten restarts' seed rows."""
    z, meta = wide
    _check_seeding(K, z, meta, (name,))


def _check_seeding(K, z, meta, names):
    for name in names:
        c = meta["cases"][name]
        x, _ = CR.case_inputs(z, meta, name)
        k = c["k"]
        got = _np(K.kmeans(x, k, max_iter=1)["seed_indices"])
        xc, _, _ = CR.prepare(x)
        first, u = CR.draws(x.shape[0], k, 10, 42)
        want = np.stack([CR.seed_one(xc, k, first[r], u[r]) for r in range(10)])
        assert got.shape == (10, k)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        assert np.array_equal(got[0], z[f"{name}/seeds0"]), name


def test_lloyd_iterations_match_the_restatement(K, golden):
    """From an explicit init, the labels after each of the first iterations (max_iter = m ends with an assign to the centres of m
    updates), n_iter and the final partition; on the relocation case (two clusters start empty) and the tolerance-stop case."""
    z, meta = golden
    for name, c in meta["cases_init"].items():
        x, init = z[f"{name}/x"], z[f"{name}/init"]
        for m in (1, 2, 3):
            want = CR.kmeans(x, c["k"], init=init, tol=c["tol"], max_iter=m)
            got = K.kmeans(x, c["k"], init=init, tol=c["tol"], max_iter=m)
            assert np.array_equal(_np(got["labels"]), want["labels"]), (name, m, int((_np(got["labels"]) != want["labels"]).sum()))
            assert got["n_iter"] == want["n_iter"] and got["best_init"] == 0
            assert np.abs(_np(got["centers"]) - want["centers"]).max() <= 1e-5 * max(1.0, np.abs(want["centers"]).max()), (name, m)
        info = {}
        want = CR.kmeans(x, c["k"], init=init, tol=c["tol"], info=info)
        got = K.kmeans(x, c["k"], init=init, tol=c["tol"])
        assert info["strict"] == c["strict"]
        assert got["n_iter"] == want["n_iter"] == c["n_iter"], (name, got["n_iter"], want["n_iter"], c["n_iter"])
        assert CR.same_partition(_np(got["labels"]), z[f"{name}/km_labels"]), name
        assert np.array_equal(_np(got["labels"]), want["labels"]), name
        assert (_np(got["seed_indices"]) == -1).all()
    # the relocation really happened: two of the six clusters are empty after the first assign, and none at the end
    x, init = z["relocate/x"], z["relocate/init"]
    xc, mean, _ = CR.prepare(x)
    first_assign = CR.assign(xc, init - mean)[0]
    assert (np.bincount(first_assign, minlength=6) == 0).sum() == 2
    assert np.bincount(_np(K.kmeans(x, 6, init=init)["labels"]), minlength=6).min() > 0


def test_assign_epilogue_paths_match_the_restatement(K, golden):
    """The assign kernel reduces a row over 32-column groups; with kpad = 64 (k = 40) a wave's two groups belong to one restart and are
    merged in the lane, with kpad = 96 (k = 70) and kpad = 32 (k = 20) they straddle restarts.  Labels after one and two iterations from
    an explicit init, and the lock-step restarts against the same restarts run one at a time (bit for bit)."""
    z, meta = golden
    x, _ = CR.case_inputs(z, meta, "set12")
    for k in (20, 40, 70):
        init = x[np.random.default_rng(k).choice(x.shape[0], size=k, replace=False)]
        for m in (1, 2):
            want, got = CR.kmeans(x, k, init=init, max_iter=m), K.kmeans(x, k, init=init, max_iter=m)
            assert np.array_equal(_np(got["labels"]), want["labels"]), (k, m, int((_np(got["labels"]) != want["labels"]).sum()))
        lock = K.kmeans(x, k, n_init=4, max_iter=20)
        rs = np.random.RandomState(42)
        for r in range(4):
            one = K.kmeans(x, k, n_init=1, max_iter=20, random_state=rs)
            assert torch.equal(one["seed_indices"][0], lock["seed_indices"][r]), (k, r)
            assert float(one["inertias"][0]) == float(lock["inertias"][r]) and int(one["n_iters"][0]) == int(lock["n_iters"][r]), (k, r)


EPILOGUE_WIDE = {130: 130, 160: 160, 257: 258}      # k -> data seed of CR.separated(seed, k, 3, 16); tests/test_clustering_cpu.py asserts the margin


def test_assign_epilogue_paths_across_column_tiles(K):
    """clus_assign_kernel with k > 128: kpad = 160 (k = 130, 160) and 288 (k = 257), so ONE restart's centres lie in two or three
    128-column tiles, whose partial minima meet only in the 64-bit atomicMin, and with n_init = 4 the restart boundaries (multiples of
    kpad) and the tile boundaries (multiples of 128) fall at different columns: waves with one_restart and waves that straddle two
    restarts (rst[1]) in the same launch.  Labels after one and two iterations from an explicit init equal the restatement's on every
    point (about three points per well-separated class: a margin of >= 1e-4 between nearest and second-nearest centre, asserted on the
    CPU), and the lock-step restarts equal the same restarts run one at a time, bit for bit."""
    for k, seed in EPILOGUE_WIDE.items():
        x, _ = CR.separated(seed, k, 3, 16)
        init = x[np.random.default_rng(k).choice(x.shape[0], size=k, replace=False)]
        for m in (1, 2):
            want, got = CR.kmeans(x, k, init=init, max_iter=m), K.kmeans(x, k, init=init, max_iter=m)
            assert np.array_equal(_np(got["labels"]), want["labels"]), (k, m, int((_np(got["labels"]) != want["labels"]).sum()))
            assert got["n_iter"] == want["n_iter"], (k, m)
        lock = K.kmeans(x, k, n_init=4, max_iter=20)
        rs = np.random.RandomState(42)
        for r in range(4):
            one = K.kmeans(x, k, n_init=1, max_iter=20, random_state=rs)
            assert torch.equal(one["seed_indices"][0], lock["seed_indices"][r]), (k, r)
            assert float(one["inertias"][0]) == float(lock["inertias"][r]) and int(one["n_iters"][0]) == int(lock["n_iters"][r]), (k, r)
            if r == lock["best_init"]:
                assert torch.equal(one["labels"], lock["labels"]) and torch.equal(one["centers"], lock["centers"]), (k, r)


def test_k_1100_seeds_and_first_iteration(K):
    """k = 1100 >= 1097: trials_of(k) = 9 (the largest count any test reaches), kpad = 1120 = 8.75 assign tiles per restart, two restarts
    in lock-step.  Both restarts' seed rows equal the restatement's; the winner (the restatement's inertias are 1.4e-3 apart, asserted
    on the CPU) and its labels after one iteration equal the restatement's, and so do the labels of either restart run alone from its
    seed rows as an explicit init."""
    k = 1100
    x, _ = CR.separated(7, k, 3, 16)
    want = CR.kmeans(x, k, n_init=2, max_iter=1)
    got = K.kmeans(x, k, n_init=2, max_iter=1)
    assert K._trials(k) == 9
    seeds = _np(got["seed_indices"])
    assert seeds.shape == (2, k) and np.array_equal(seeds, want["seed_indices"]), np.argwhere(seeds != want["seed_indices"])[:5]
    rel = np.abs(_np(got["inertias"]) - want["inertias"]) / want["inertias"]
    print(f"[clustering] k=1100: per-restart inertia, device - restatement (relative) {rel}, best_init {got['best_init']}")
    assert got["best_init"] == want["best_init"] and (rel <= 1e-5).all()
    assert np.array_equal(_np(got["labels"]), want["labels"]), int((_np(got["labels"]) != want["labels"]).sum())
    for r in range(2):
        alone = K.kmeans(x, k, init=x[want["seed_indices"][r]], max_iter=1)
        assert np.array_equal(_np(alone["labels"]), want["all_labels"][r]), (r, int((_np(alone["labels"]) != want["all_labels"][r]).sum()))


@pytest.mark.parametrize("k,copies,per,d,seed", [(160, 20, 5, 16, 99), (12, 3, 8, 1100, 98)])
def test_relocation_of_many_empty_clusters(K, k, copies, per, d, seed):
    """clus_relocate_kernel moving several points in one iteration: `copies` of the k explicit centres are the same data point, so after
    the first assign copies - 1 clusters are empty (the first copy wins every tie) and as many points, farthest first, become centres.
    At k = 160 that is 19 of 160 in one iteration (kpad = 160: two assign tiles); at D = 1100 (dpad 1120) the sums are moved in two trips
    of the kernel's c += 1024 loop.  Labels, cluster sizes, n_iter and centres after iterations 1 - 3 against the restatement."""
    x, _ = CR.separated(seed, k, per, d)
    init = CR.duplicate_init(x, k, copies, 5)
    xc, mean, _ = CR.prepare(x)
    first_assign = CR.assign(xc, init - mean)[0]
    assert (np.bincount(first_assign, minlength=k) == 0).sum() == copies - 1
    for m in (1, 2, 3):
        want, got = CR.kmeans(x, k, init=init, max_iter=m), K.kmeans(x, k, init=init, max_iter=m)
        lab = _np(got["labels"])
        assert np.array_equal(lab, want["labels"]), (m, int((lab != want["labels"]).sum()))
        assert np.array_equal(np.bincount(lab, minlength=k), np.bincount(want["labels"], minlength=k)), m
        assert got["n_iter"] == want["n_iter"] and got["best_init"] == 0
        assert np.abs(_np(got["centers"]) - want["centers"]).max() <= 1e-5 * max(1.0, np.abs(want["centers"]).max()), m
    assert np.bincount(_np(K.kmeans(x, k, init=init)["labels"]), minlength=k).min() > 0


def test_scores_kernel_on_a_large_table(K, wide):
    """clus_contingency_kernel / clus_scores_kernel on 20 000 labels with about 300 x 350 occupied classes (the goldens have at most
    30 x 30): within 1e-12 of the restatement, which tests/test_clustering_cpu.py pins to sklearn.metrics on this very table."""
    _, meta = wide
    rec = meta["scores_table"]
    a, b = CR.label_pair(**rec["gen"])
    assert CR.sha256(a, b) == rec["sha256"] and (np.unique(a).size, np.unique(b).size) == (rec["classes_true"], rec["classes_pred"])
    want = CR.scores(a, b)
    for ta, tb in ((a, b), (torch.from_numpy(a).cuda(), torch.from_numpy(b.astype(np.int32)).cuda()), (a * 3 - 400, 10000 - 7 * b)):
        got = K.clustering_scores(ta, tb)
        err = max(abs(got["ari"] - want[0]), abs(got["nmi"] - want[1]), abs(got["v_measure"] - want[2]))
        print(f"[clustering] scores on a {rec['classes_true']} x {rec['classes_pred']} table: device {got}, max error {err:.3e}")
        assert err <= 1e-12, (got, want)
        assert max(abs(got["ari"] - rec["ari"]), abs(got["nmi"] - rec["nmi"]), abs(got["v_measure"] - rec["v_measure"])) <= 1e-12


def test_winning_restart_and_per_restart_results(K, golden):
    z, meta = golden
    for name in ("set8", "set12", "set30_d100"):
        c = meta["cases"][name]
        x, _ = CR.case_inputs(z, meta, name)
        km = K.kmeans(x, c["k"])
        assert km["best_init"] == c["restatement_best_init"], name
        inert = _np(km["inertias"])
        assert inert.shape == (10,) and km["inertia"] == inert[km["best_init"]] == inert.min()
        print(f"[clustering] {name}: per-restart inertia, device - restatement (relative) "
              f"{np.array2string((inert - np.array(c['restatement_inertias'])) / inert, precision=2)}")
        assert abs(km["inertia"] - c["inertia"]) <= 1e-5 * c["inertia"], name
        assert _np(km["n_iters"])[km["best_init"]] == km["n_iter"]


def test_inertia_against_fp64_recomputation(K, golden):
    """inertia = sum_i sum_c (xc[i, c] - centre[label_i, c])^2 with xc = fp32(x - mean): per element the subtraction rounds once
    (relative u = 2^-24 of the difference), the square once, and the D terms are added one after the other in fp32 (each partial sum
    rounds once: <= (D - 1) u relative, all terms being non-negative); the sum over points is fp64.  So relative to the same expression
    in fp64, |error| <= (D + 2) u (1 + small).  The returned centres carry the mean again (one more rounding of |centre + mean| u per
    element), which moves each difference by at most u (|centre| + |mean|) and the total by sum 2 |diff| u (|centre| + |mean|)."""
    z, meta = golden
    _check_inertia(K, z, meta, ("set8", "set20_d768", "set30_d100"))


def test_inertia_of_the_wide_cases_against_fp64_recomputation(K, wide):
    """clus_inertia_kernel and clus_export_kernel at D = 1280 and 1536; the bound above is already a function of D."""
    z, meta = wide
    _check_inertia(K, z, meta, ("wide8_d1280", "wide10_d1536"))


def _check_inertia(K, z, meta, names):
    u = 2.0 ** -24
    for name in names:
        c = meta["cases"][name]
        x, _ = CR.case_inputs(z, meta, name)
        km = K.kmeans(x, c["k"])
        lab, centres = _np(km["labels"]), _np(km["centers"]).astype(np.float64)
        xc, mean, _ = CR.prepare(x)
        diff = xc.astype(np.float64) - (centres[lab] - mean.astype(np.float64))
        want = float((diff ** 2).sum())
        slack = float((2.0 * np.abs(diff) * u * (np.abs(centres[lab]) + np.abs(mean.astype(np.float64)) * 2.0)).sum())
        bound = (x.shape[1] + 2) * u * want * 1.01 + slack
        print(f"[clustering] {name}: inertia {km['inertia']!r} fp64 {want!r} rel {abs(km['inertia'] - want) / want:.3e} bound {bound / want:.3e}")
        assert abs(km["inertia"] - want) <= bound, name


def test_scores_kernel_against_the_golden(K, golden):
    z, meta = golden
    for name, c in meta["cases"].items():
        if f"{name}/km_labels" not in z:
            continue
        _, lab = CR.case_inputs(z, meta, name)
        true = CR.reduce_labels(lab).astype(np.int64)
        pred = z[f"{name}/km_labels"].astype(np.int64)
        ref = c["eval_clustering"]
        for a, b in ((true, pred), (true.astype(np.int32), torch.from_numpy(pred.astype(np.int32)).cuda()), (true * 7 - 50, 1000 - 3 * pred)):
            got = K.clustering_scores(a, b)
            assert abs(got["ari"] - ref["clustering_ari"]) <= 1e-12 and abs(got["nmi"] - ref["clustering_nmi"]) <= 1e-12, name
            assert abs(got["v_measure"] - ref["clustering_v_measure"]) <= 1e-12, name
    # the degenerate corners, by the restatement (pinned to sklearn.metrics in tests/test_clustering_cpu.py)
    for a, b in (([0, 0, 0, 0], [1, 1, 1, 1]), ([0, 0, 1, 1], [5, 5, 5, 5]), ([0, 1, 2, 3], [0, 1, 2, 3]), ([0, 0, 0, 0], [0, 1, 2, 3]),
                 ([0, 1, 0, 1], [0, 0, 1, 1]), ([3], [9])):
        got, want = K.clustering_scores(np.array(a), np.array(b)), CR.scores(a, b)
        assert max(abs(got["ari"] - want[0]), abs(got["nmi"] - want[1]), abs(got["v_measure"] - want[2])) <= 1e-12, (a, b, got, want)


def test_bit_reproducible_and_independent_of_where_the_inputs_live(K, golden):
    z, meta = golden
    x, lab = CR.case_inputs(z, meta, "set12")
    k = meta["cases"]["set12"]["k"]
    xd = torch.from_numpy(x).cuda()
    a, b, host = K.kmeans(xd, k), K.kmeans(xd, k), K.kmeans(x, k)
    for other in (b, host):
        assert torch.equal(a["labels"], other["labels"]) and torch.equal(a["centers"], other["centers"])
        assert torch.equal(a["inertias"], other["inertias"]) and a["inertia"] == other["inertia"]
        assert torch.equal(a["seed_indices"], other["seed_indices"]) and torch.equal(a["n_iters"], other["n_iters"])
    # fp64 inputs are computed in fp32: the same bits again
    c = K.kmeans(x.astype(np.float64), k)
    assert torch.equal(a["labels"], c["labels"]) and a["inertia"] == c["inertia"]
    # a row-strided view is read in place, a column-strided one through a copy: the same result as the contiguous matrix
    wide = torch.zeros((x.shape[0], x.shape[1] + 9), device="cuda")
    wide[:, : x.shape[1]] = xd
    d = K.kmeans(wide[:, : x.shape[1]], k)
    assert torch.equal(a["labels"], d["labels"]) and a["inertia"] == d["inertia"]
    twice = torch.zeros((x.shape[0], 2 * x.shape[1]), device="cuda")
    twice[:, ::2] = xd
    e = K.kmeans(twice[:, ::2], k)
    assert torch.equal(a["labels"], e["labels"]) and a["inertia"] == e["inertia"]
    assert K.eval_clustering(xd, torch.from_numpy(lab).cuda()) == K.eval_clustering(x, lab)


def test_nan_input_gives_zeros_and_limits_raise(K, golden):
    z, meta = golden
    x, lab = CR.case_inputs(z, meta, "nan_row")
    assert np.isnan(x).any()
    assert K.eval_clustering(x, lab) == CR.ZERO == meta["cases"]["nan_row"]["eval_clustering"]
    x2 = x.copy()
    x2[np.isnan(x2)] = np.inf
    assert K.eval_clustering(torch.from_numpy(x2).cuda(), lab) == CR.ZERO
    assert K.kmeans(x, 3)["finite"] is False and K.kmeans(np.nan_to_num(x), 3)["finite"] is True
    with pytest.raises(ValueError, match="limit of 4096"):
        K.kmeans(np.zeros((5000, 4), dtype=np.float32), 4097)
    with pytest.raises(ValueError, match="limit of 4096"):
        K.eval_clustering(np.zeros((5000, 4), dtype=np.float32), np.arange(5000), n_clusters=4097)
    with pytest.raises(ValueError, match="n_init"):
        K.kmeans(np.zeros((50, 4), dtype=np.float32), 3, n_init=65)
