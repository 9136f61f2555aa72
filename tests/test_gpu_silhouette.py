"""The device silhouette (avex_amd.clustering.silhouette_samples / silhouette_score, csrc/silhouette.hip) against scikit-learn's float64
result on the same fp32 inputs (tests/golden/silhouette.npz, made by tests/golden/make_silhouette_goldens.py).  Nothing here needs
scikit-learn or the reference tree.

Tolerances: 1e-6 per sample, 1e-7 on the score.  Their basis is a NumPy emulation of this arithmetic (fp32 Gram form on centred /
normalised rows, fp64 cluster sums), which stayed within 4.2e-8 / 4.7e-10 (Euclidean) and 6.9e-8 / 1.2e-9 (cosine) of the float64
result: the bars leave at least 14 x for the MFMA's summation order.  Every test prints what the device gave before it asserts."""
import numpy as np
import pytest
import torch

import _clustering_ref as CR
import _silhouette_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return SR.load_golden(golden_dir)


@pytest.fixture(scope="module")
def wide(golden_dir):
    return CR.load_wide(golden_dir)


@pytest.fixture(scope="module")
def K(built_lib):
    from avex_amd import clustering
    return clustering


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("metric", SR.METRICS)
@pytest.mark.parametrize("name", list(SR.CASES))
def test_golden_case(K, golden, name, metric):
    z, meta = golden
    x, lab = SR.case_inputs(name)
    got = K.silhouette_samples(x, lab, metric=metric)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],)
    score = K.silhouette_score(x, lab, metric=metric)
    err = float(np.abs(_np(got) - z[f"{name}/{metric}"]).max())
    score_err = abs(score - meta["cases"][name]["score"][metric])
    print(f"[silhouette] {name} {metric}: per sample {err:.3e}, score {score_err:.3e} (device {score!r})")
    assert isinstance(score, float)
    assert err <= SR.TOL_SAMPLE, (name, metric, err)
    assert score_err <= SR.TOL_SCORE, (name, metric, score_err)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_sample_size_follows_scikit_learn(K, golden, metric):
    z, meta = golden
    for rec in meta["sampled"]:
        x, lab = SR.case_inputs(rec["case"])
        got = K.silhouette_score(torch.from_numpy(x).cuda(), lab, metric=metric, sample_size=rec["sample_size"], random_state=rec["random_state"])
        err = abs(got - rec["score"][metric])
        print(f"[silhouette] {rec['case']} sample {rec['sample_size']} seed {rec['random_state']} {metric}: score {err:.3e}")
        assert err <= SR.TOL_SCORE, (rec, metric, got)
        idx = z[f"{rec['case']}/sample{rec['sample_size']}_seed{rec['random_state']}/indices"]
        sub = K.silhouette_samples(x[idx], lab[idx], metric=metric)
        want = z[f"{rec['case']}/sample{rec['sample_size']}_seed{rec['random_state']}/{metric}"]
        assert float(np.abs(_np(sub) - want).max()) <= SR.TOL_SAMPLE
        assert abs(got - float(_np(sub).mean())) <= 1e-14
    # the label count is checked on the subsample: 130 points with 129 labels; seed 3 draws 100 points with 100 labels, seed 1 with 99
    x, lab = SR.case_inputs("k_n_minus_1")
    assert np.unique(lab[SR.sample_indices(130, 100, 3)]).size == 100 and np.unique(lab[SR.sample_indices(130, 100, 1)]).size == 99
    with pytest.raises(ValueError, match=r"^Number of labels is 100\. Valid values are 2 to n_samples - 1 \(inclusive\)$"):
        K.silhouette_score(x, lab, metric=metric, sample_size=100, random_state=3)
    assert isinstance(K.silhouette_score(x, lab, metric=metric, sample_size=100, random_state=1), float)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_bit_for_bit_equal(K, metric):
    """The per-cluster sums are 64-bit integers (fixed point) added with integer atomics: no order can change them."""
    x, lab = SR.case_inputs("c300")
    base = K.silhouette_samples(x, lab, metric=metric)
    base_score = K.silhouette_score(x, lab, metric=metric)
    for batch_size in (64, 128, 2048):
        other = K.silhouette_samples(x, lab, metric=metric, batch_size=batch_size)
        assert torch.equal(base, other), (metric, batch_size, float((base - other).abs().max()))
        assert K.silhouette_score(x, lab, metric=metric, batch_size=batch_size) == base_score
    xd, labd = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    assert torch.equal(base, K.silhouette_samples(xd, labd, metric=metric))                       # host against device inputs
    assert torch.equal(base, K.silhouette_samples(xd, lab, metric=metric))
    assert torch.equal(base, K.silhouette_samples(x.astype(np.float64), lab, metric=metric))      # fp64 X is computed in fp32
    assert torch.equal(base, K.silhouette_samples(xd.double(), labd.to(torch.int32), metric=metric))
    assert torch.equal(base, K.silhouette_samples(x, lab, metric=metric))                         # two successive runs
    assert K.silhouette_score(xd, labd, metric=metric) == base_score
    # a larger set with more than one row tile, column segment and batch
    x, lab = SR.case_inputs("c2000_d768")
    a, b = K.silhouette_samples(x, lab, metric=metric), K.silhouette_samples(x, lab, metric=metric, batch_size=384)
    assert torch.equal(a, b)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_duplicates_and_singletons(K, golden, metric):
    x, lab = SR.case_inputs("duplicates")
    s = _np(K.silhouette_samples(x, lab, metric=metric))
    rows = lab == 2
    print(f"[silhouette] duplicates {metric}: max |s - 1| over the cluster of copies {np.abs(s[rows] - 1.0).max():.3e}")
    assert np.abs(s[rows] - 1.0).max() <= 1e-6
    if metric == "euclidean":                      # the norms come from the same product as the Gram entries: a == 0 exactly
        assert (s[rows] == 1.0).all()
    x, lab = SR.case_inputs("singletons")
    s = _np(K.silhouette_samples(x, lab, metric=metric))
    alone = np.bincount(lab)[lab] == 1
    assert alone.sum() == 5 and (s[alone] == 0.0).all() and (s[~alone] != 0.0).all()
    x, lab = SR.case_inputs("k_n_minus_1")
    s = _np(K.silhouette_samples(x, lab, metric=metric))
    assert (s[1:129] == 0.0).all() and s[0] != 0.0 and s[129] != 0.0


def test_label_kinds_give_the_same_result(K):
    x, lab = SR.case_inputs("int_labels")
    base = K.silhouette_samples(x, lab)
    dense = np.unique(lab, return_inverse=True)[1]
    for other in (dense, dense.astype(np.int32), torch.from_numpy(lab).cuda(), np.array(["a", "b", "c"])[dense], 10.0 * dense - 5.0):
        assert torch.equal(base, K.silhouette_samples(x, other))


def test_eval_clustering_with_silhouette(K, golden_dir):
    z, meta = CR.load_golden(golden_dir)
    name = "set30_d100"
    x, lab = CR.case_inputs(z, meta, name)
    plain = K.eval_clustering(x, lab)
    got = K.eval_clustering_silhouette(x, lab)
    print(f"[silhouette] eval_clustering_silhouette {name}: {got}")
    assert set(plain) == {"clustering_ari", "clustering_nmi", "clustering_v_measure"} and set(got) == set(plain) | {"clustering_silhouette"}
    for key, v in plain.items():
        assert abs(got[key] - v) <= 1e-12 and abs(v - meta["cases"][name]["eval_clustering"][key]) <= 1e-12, key
    km = K.kmeans(x, meta["cases"][name]["k"])
    assert got["clustering_silhouette"] == K.silhouette_score(x, km["labels"])
    assert abs(got["clustering_silhouette"] - SR.silhouette_score(x, _np(km["labels"]))) <= SR.TOL_SCORE
    assert K.eval_clustering_silhouette(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()) == got


# ------------------------------------------------------------------------------------------------------------------------------
#  Past the shapes of silhouette.npz (SR.WIDE_CASES, expected values in tests/golden/metrics_wide.npz): D = 1280 and 1536 (the K loop of
#  the shared fp32 tile runs 40 / 48 steps and the centring pass of clustering.hip takes its second column block), 200 and 1005 labels
#  (n_slots grows by up to 31 padding slots per label: 3041 points occupy 32 256 slots, so most row tiles and column segments of the
#  product are padding next to two to four live rows), and more than one batch at those sizes.  The bars follow the header's rule case by
#  case: the constant where it leaves 14 x the recorded error of the NumPy emulation, 14 x that error otherwise (SR.wide_bars).
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", SR.METRICS)
@pytest.mark.parametrize("name", list(SR.WIDE_CASES))
def test_wide_golden_case(K, wide, name, metric):
    z, meta = wide
    rec = meta["silhouette"]["cases"][name]
    x, lab = SR.case_inputs(name)
    assert (x.shape[0], x.shape[1], np.unique(lab).size) == (rec["n"], rec["d"], rec["k"])
    bar, score_bar = SR.wide_bars(rec, metric)
    got = K.silhouette_samples(x, lab, metric=metric)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],)
    score = K.silhouette_score(x, lab, metric=metric)
    err = float(np.abs(_np(got) - z[f"sil/{name}/{metric}"]).max())
    score_err = abs(score - rec["score"][metric])
    print(f"[silhouette] {name} {metric}: per sample {err:.3e} (bar {bar:.3e}, emulation {rec['restatement_max_err'][metric]:.3e}), "
          f"score {score_err:.3e} (bar {score_bar:.3e}, emulation {rec['restatement_score_err'][metric]:.3e}, device {score!r})")
    assert isinstance(score, float)
    assert err <= bar, (name, metric, err, bar)
    assert score_err <= score_bar, (name, metric, score_err, score_bar)


@pytest.mark.parametrize("metric", SR.METRICS)
def test_bit_for_bit_equal_at_200_labels_and_d1280(K, metric):
    """2600 points, 200 labels, D = 1280 (about 7 400 slots): one batch (2048 slots and more), several (384) and many (128), host and
    device inputs -- the integer sums make every one of them the same bits."""
    x, lab = SR.case_inputs("w2600_d1280_k200")
    base = K.silhouette_samples(x, lab, metric=metric)
    base_score = K.silhouette_score(x, lab, metric=metric)
    for batch_size in (128, 384, 2048):
        other = K.silhouette_samples(x, lab, metric=metric, batch_size=batch_size)
        assert torch.equal(base, other), (metric, batch_size, float((base - other).abs().max()))
        assert K.silhouette_score(x, lab, metric=metric, batch_size=batch_size) == base_score
    xd, labd = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    assert torch.equal(base, K.silhouette_samples(xd, labd, metric=metric, batch_size=384))
    assert torch.equal(base, K.silhouette_samples(xd, lab, metric=metric))
    assert K.silhouette_score(xd, labd, metric=metric) == base_score


@pytest.mark.parametrize("metric", SR.METRICS)
def test_singletons_among_a_thousand_labels(K, wide, metric):
    """1000 labels of two to four points and five of one: a point alone in its cluster scores exactly 0.0, every other one does not, and
    several batches change nothing."""
    z, _ = wide
    x, lab = SR.case_inputs("many_labels_k1005")
    s = _np(K.silhouette_samples(x, lab, metric=metric))
    alone = np.bincount(lab)[lab] == 1
    assert alone.sum() == 5 and (s[alone] == 0.0).all() and (s[~alone] != 0.0).all()
    assert (z[f"sil/many_labels_k1005/{metric}"][alone] == 0.0).all()
    assert np.array_equal(s, _np(K.silhouette_samples(x, lab, metric=metric, batch_size=4096)))


def test_eval_clustering_with_silhouette_on_wide_rows(K, wide):
    """eval_clustering_silhouette at D = 1280: the silhouette kernels read the rows the clustering kernels centred (ld = dpad = 1280).  The
    three scores are the reference's within 1e-12; the silhouette column is scikit-learn's float64 score of scikit-learn's own k-means
    partition -- the same partition, as test_gpu_clustering.py checks -- within the bar of its recorded emulation error."""
    z, meta = wide
    rec = meta["eval_silhouette"]
    name = rec["case"]
    x, lab = CR.case_inputs(z, meta, name)
    got = K.eval_clustering_silhouette(x, lab)
    print(f"[silhouette] eval_clustering_silhouette {name}: {got}")
    for key, v in meta["cases"][name]["eval_clustering"].items():
        assert abs(got[key] - v) <= 1e-12, (key, got[key], v)
    _, score_bar = SR.wide_bars(rec, "euclidean")
    err = abs(got["clustering_silhouette"] - rec["score"])
    print(f"[silhouette] eval_clustering_silhouette {name}: silhouette error {err:.3e} (bar {score_bar:.3e}, emulation {rec['restatement_score_err']['euclidean']:.3e})")
    assert err <= score_bar, (err, score_bar)
    km = K.kmeans(x, meta["cases"][name]["k"])
    assert CR.same_partition(_np(km["labels"]), z[f"{name}/km_labels"])
    assert got["clustering_silhouette"] == K.silhouette_score(x, km["labels"])


def test_eval_clustering_multiple_k_with_silhouette(K, golden_dir):
    z, meta = CR.load_golden(golden_dir)
    x, lab = CR.case_inputs(z, meta, "set30_d100")
    x, lab = x[:600], lab[:600]
    plain = K.eval_clustering_multiple_k(x, lab, k_range=(28, 30))
    got = K.eval_clustering_multiple_k_silhouette(x, lab, k_range=(28, 30))
    print(f"[silhouette] eval_clustering_multiple_k_silhouette: {got}")
    assert set(got) == set(plain) | {"clustering_silhouette_best"}
    for key, v in plain.items():
        assert abs(got[key] - v) <= 1e-12, key
    k = int(got["clustering_best_k"])
    assert got["clustering_silhouette_best"] == K.eval_clustering_silhouette(x, lab, n_clusters=k)["clustering_silhouette"]
    assert got["clustering_silhouette_best"] == K.silhouette_score(x, K.kmeans(x, k)["labels"])


def test_non_finite_input_and_the_value_errors(K):
    x, lab = SR.case_inputs("c300")
    for bad in (np.nan, np.inf, -np.inf):
        x2 = x.copy()
        x2[17, 3] = bad
        for metric in SR.METRICS:
            with pytest.raises(ValueError, match="Input X contains NaN or infinity"):
                K.silhouette_samples(x2, lab, metric=metric)
            with pytest.raises(ValueError, match="Input X contains NaN or infinity"):
                K.silhouette_score(torch.from_numpy(x2).cuda(), lab, metric=metric)
        zero = {"clustering_ari": 0.0, "clustering_nmi": 0.0, "clustering_v_measure": 0.0, "clustering_silhouette": 0.0}
        assert K.eval_clustering_silhouette(x2, lab) == zero
    assert K.eval_clustering_silhouette(x, np.zeros_like(lab)) == {"clustering_ari": 0.0, "clustering_nmi": 0.0, "clustering_v_measure": 0.0,
                                                                   "clustering_silhouette": 0.0}
    with pytest.raises(ValueError, match=r"^Number of labels is 1\. Valid values are 2 to n_samples - 1 \(inclusive\)$"):
        K.silhouette_samples(x, np.zeros_like(lab))
    with pytest.raises(ValueError, match=r"^Number of labels is 300\. Valid values are 2 to n_samples - 1 \(inclusive\)$"):
        K.silhouette_score(x, np.arange(300))
    with pytest.raises(ValueError, match="limit of 4096"):
        K.silhouette_score(np.zeros((5000, 4), dtype=np.float32), np.arange(5000) % 4097)
    with pytest.raises(ValueError, match="metric must be"):
        K.silhouette_samples(x, lab, metric="precomputed")
