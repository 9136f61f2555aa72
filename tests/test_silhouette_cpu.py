"""The silhouette functions of avex_amd.clustering without a GPU: the NumPy restatement of the device arithmetic
(tests/_silhouette_ref.py) against scikit-learn's float64 result (tests/golden/silhouette.npz, written by
tests/golden/make_silhouette_goldens.py) inside the tolerances the device has to meet, and the module's contract -- signatures, the
ValueError cases and texts, the subsample draw, the C struct mirror, the exported symbols, the unchanged reference functions."""
import inspect
import os

import numpy as np
import pytest
import torch

import _clustering_ref as CR
import _silhouette_ref as SR
from avex_amd import _capi
from avex_amd import clustering as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return SR.load_golden(golden_dir)


def test_golden_covers_the_cases(golden):
    z, meta = golden
    c = meta["cases"]
    assert set(c) == set(SR.CASES)
    shape = {name: (m["n"], m["d"], m["k"]) for name, m in c.items()}
    assert shape["c300"] == (300, 40, 5) and shape["c515_offset"] == (515, 37, 7)
    assert shape["c1000_d768"] == (1000, 768, 12) and shape["c2000_d768"] == (2000, 768, 30)
    assert shape["k2"][2] == 2 and shape["k_n_minus_1"] == (130, 16, 129)
    assert set(np.unique(SR.case_inputs("int_labels")[1]).tolist()) == {-3, 7, 1000}
    assert SR.case_inputs("str_labels")[1].dtype.kind == "U"
    x, lab = SR.case_inputs("c515_offset")
    assert abs(float(x.mean()) - 50.0) < 10.0 and float(x.std()) > 100.0
    assert (np.bincount(SR.case_inputs("singletons")[1]) == 1).sum() == 5
    assert sorted(np.bincount(SR.case_inputs("sizes_31_129")[1]).tolist()) == [31, 32, 33, 127, 128, 129]
    x, lab = SR.case_inputs("duplicates")
    assert (x[lab == 2] == x[lab == 2][0]).all() and (lab == 2).sum() > 32 and c["duplicates"]["conditions"]["identical_pairs"] > 0
    for name, m in c.items():
        assert m["conditions"]["min_separation_over_rms"] >= meta["min_separation"] == 1e-2, name
        assert m["conditions"]["mean_cosine_distance"] >= meta["min_mean_cosine_distance"] == 0.5, name
        for metric in SR.METRICS:
            assert z[f"{name}/{metric}"].dtype == np.float64 and z[f"{name}/{metric}"].shape == (m["n"],)
    assert [(r["case"], r["sample_size"], r["random_state"]) for r in meta["sampled"]] == [("c515_offset", 200, 0), ("c515_offset", 200, 7)]
    assert (meta["tol_sample"], meta["tol_score"]) == (SR.TOL_SAMPLE, SR.TOL_SCORE) == (1e-6, 1e-7)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "silhouette.npz")) < 1 << 20


@pytest.mark.parametrize("metric", SR.METRICS)
def test_restatement_reproduces_every_golden(golden, metric):
    z, meta = golden
    for name, m in meta["cases"].items():
        x, lab = SR.case_inputs(name)
        got = SR.silhouette_samples(x, lab, metric)
        err = float(np.abs(got - z[f"{name}/{metric}"]).max())
        score_err = abs(float(got.sum() / got.shape[0]) - m["score"][metric])
        print(f"[silhouette] restatement {name} {metric}: per sample {err:.2e}, score {score_err:.2e}")
        assert err <= SR.TOL_SAMPLE and score_err <= SR.TOL_SCORE, (name, metric, err, score_err)
    for rec in meta["sampled"]:
        x, lab = SR.case_inputs(rec["case"])
        got = SR.silhouette_score(x, lab, metric, sample_size=rec["sample_size"], random_state=rec["random_state"])
        assert abs(got - rec["score"][metric]) <= SR.TOL_SCORE, (rec, metric, got)


# ------------------------------------------------------------------------------------------------------------------------------
#  Past the shapes of silhouette.npz: SR.WIDE_CASES against tests/golden/metrics_wide.npz
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(golden_dir):
    return CR.load_wide(golden_dir)


def test_wide_golden_covers_the_cases(wide):
    z, meta = wide
    sil = meta["silhouette"]
    assert set(sil["cases"]) == set(SR.WIDE_CASES) and not set(SR.WIDE_CASES) & set(SR.CASES)
    assert (sil["tol_sample"], sil["tol_score"], sil["mfma_margin"]) == (SR.TOL_SAMPLE, SR.TOL_SCORE, SR.MFMA_MARGIN) == (1e-6, 1e-7, 14.0)
    shape = {name: (m["n"], m["d"], m["k"]) for name, m in sil["cases"].items()}
    assert shape["w2600_d1280_k200"] == (2600, 1280, 200) and shape["w400_d1536"] == (400, 1536, 6) and shape["many_labels_k1005"][1:] == (24, 1005)
    sizes = np.bincount(SR.case_inputs("many_labels_k1005")[1])
    assert (sizes == 1).sum() == 5 and sizes.max() == 4 and ((sizes >= 2) & (sizes <= 4)).sum() == 1000
    for name, m in sil["cases"].items():
        assert m["conditions"]["min_separation_over_rms"] >= 1e-2 and m["conditions"]["mean_cosine_distance"] >= 0.5, name
        for metric in SR.METRICS:
            assert z[f"sil/{name}/{metric}"].dtype == np.float64 and z[f"sil/{name}/{metric}"].shape == (m["n"],)
            # the bars are the constants, or 14 x the recorded emulation error where that is larger -- never below the constants
            bar, score_bar = SR.wide_bars(m, metric)
            assert bar == max(SR.TOL_SAMPLE, 14.0 * m["restatement_max_err"][metric]) and score_bar == max(SR.TOL_SCORE, 14.0 * m["restatement_score_err"][metric])
    ev = meta["eval_silhouette"]
    assert ev["case"] == "wide8_d1280" and meta["cases"][ev["case"]]["gen"]["d"] == 1280


@pytest.mark.parametrize("metric", SR.METRICS)
@pytest.mark.parametrize("name", list(SR.WIDE_CASES))
def test_restatement_reproduces_the_wide_cases(wide, name, metric):
    """The emulation's error against scikit-learn float64 IS what the generator recorded (the basis of the GPU tests' bars), and it is
    inside the bar the device has to meet with the margin left over."""
    z, meta = wide
    m = meta["silhouette"]["cases"][name]
    x, lab = SR.case_inputs(name)
    got = SR.silhouette_samples(x, lab, metric)
    err = float(np.abs(got - z[f"sil/{name}/{metric}"]).max())
    score_err = abs(float(got.sum() / got.shape[0]) - m["score"][metric])
    bar, score_bar = SR.wide_bars(m, metric)
    print(f"[silhouette] restatement {name} {metric}: per sample {err:.2e} (bar {bar:.2e}), score {score_err:.2e} (bar {score_bar:.2e})")
    # to 10 %: another BLAS may round a Gram entry the other way
    assert abs(err - m["restatement_max_err"][metric]) <= 0.1 * err and abs(score_err - m["restatement_score_err"][metric]) <= 0.1 * score_err
    assert SR.MFMA_MARGIN * err <= 1.1 * bar and SR.MFMA_MARGIN * score_err <= 1.1 * score_bar
    alone = np.bincount(lab)[lab] == 1
    assert (got[alone] == 0.0).all() and (z[f"sil/{name}/{metric}"][alone] == 0.0).all()


def test_restatement_on_the_wide_clustering_partition(wide):
    z, meta = wide
    ev = meta["eval_silhouette"]
    x, _ = CR.case_inputs(z, meta, ev["case"])
    km = z[f"{ev['case']}/km_labels"].astype(np.int64)
    err = abs(SR.silhouette_score(x, km) - ev["score"])
    assert abs(err - ev["restatement_score_err"]["euclidean"]) <= 0.1 * err and err <= SR.TOL_SCORE / SR.MFMA_MARGIN


def test_restatement_duplicates_and_singletons(golden):
    z, _ = golden
    x, lab = SR.case_inputs("duplicates")
    d = SR.distances(x, "euclidean")
    rows = np.flatnonzero(lab == 2)
    assert (d[np.ix_(rows, rows)] == 0.0).all()                      # exactly: the norms come from the same product as the Gram entries
    for metric in SR.METRICS:
        s = SR.silhouette_samples(x, lab, metric)
        assert np.abs(s[rows] - 1.0).max() <= 1e-6 and np.abs(z[f"duplicates/{metric}"][rows] - 1.0).max() <= 1e-12
    x, lab = SR.case_inputs("singletons")
    alone = np.bincount(lab)[lab] == 1
    for metric in SR.METRICS:
        assert (SR.silhouette_samples(x, lab, metric)[alone] == 0.0).all() and (z[f"singletons/{metric}"][alone] == 0.0).all()


def test_sample_draw_is_scikit_learns(golden):
    z, meta = golden
    for rec in meta["sampled"]:
        want = z[f"{rec['case']}/sample{rec['sample_size']}_seed{rec['random_state']}/indices"]
        n = meta["cases"][rec["case"]]["n"]
        assert np.array_equal(K._check_random_state(rec["random_state"]).permutation(n)[: rec["sample_size"]], want)
        assert np.array_equal(SR.sample_indices(n, rec["sample_size"], rec["random_state"]), want)
    rs = np.random.RandomState(3)
    assert K._check_random_state(rs) is rs and K._check_random_state(None) is np.random.mtrand._rand
    utils = pytest.importorskip("sklearn.utils")
    for seed in (0, 7, 12345):
        assert np.array_equal(K._check_random_state(seed).permutation(515)[:200], utils.check_random_state(seed).permutation(515)[:200])
    with pytest.raises(ValueError):
        K._check_random_state("seed")


def test_signatures():
    p = inspect.signature(K.silhouette_samples).parameters
    assert list(p) == ["X", "labels", "metric", "batch_size"]
    assert (p["metric"].default, p["batch_size"].default) == ("euclidean", 2048)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("metric", "batch_size"))
    p = inspect.signature(K.silhouette_score).parameters
    assert list(p)[:6] == ["X", "labels", "metric", "sample_size", "random_state", "batch_size"]
    assert [p[n].default for n in ("metric", "sample_size", "random_state", "batch_size")] == ["euclidean", None, None, 2048]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("metric", "sample_size", "random_state", "batch_size"))
    for name in ("silhouette_samples", "silhouette_score", "eval_clustering_silhouette", "eval_clustering_multiple_k_silhouette"):
        assert name in K.__all__
    # the two reference functions keep their signatures, and their empty results their keys; the silhouette variants take the same arguments
    for plain, extended in ((K.eval_clustering, K.eval_clustering_silhouette), (K.eval_clustering_multiple_k, K.eval_clustering_multiple_k_silhouette)):
        assert str(inspect.signature(plain)) == str(inspect.signature(extended))
    assert list(inspect.signature(K.eval_clustering).parameters) == ["embeds", "labels", "n_clusters", "random_state"]
    assert list(inspect.signature(K.eval_clustering_multiple_k).parameters) == ["embeds", "labels", "k_range", "random_state"]
    assert set(K._get_empty_clustering_metrics()) == {"clustering_ari", "clustering_nmi", "clustering_v_measure"}
    assert set(K._get_empty_clustering_best_metrics()) == {"clustering_best_k", "clustering_ari_best", "clustering_nmi_best", "clustering_v_measure_best"}
    assert (K.MAX_SIL_N, K.MAX_SIL_LABELS) == (524288, 4096)


def test_value_errors_that_need_no_device():
    x = np.zeros((6, 3), dtype=np.float32)
    lab = np.array([0, 0, 1, 1, 2, 2])
    for fn in (K.silhouette_samples, K.silhouette_score):
        for metric in ("precomputed", "manhattan", "l2", None):
            with pytest.raises(ValueError, match="metric must be 'euclidean' or 'cosine'"):
                fn(x, lab, metric=metric)
        with pytest.raises(ValueError, match=r"^Found input variables with inconsistent numbers of samples: \[6, 5\]$"):
            fn(x, lab[:5])
        with pytest.raises(ValueError, match=r"^Found input variables with inconsistent numbers of samples: \[6, 5\]$"):
            fn(torch.zeros(6, 3), torch.arange(5))
        with pytest.raises(ValueError, match="2D"):
            fn(np.zeros(6, dtype=np.float32), lab)
        with pytest.raises(ValueError, match="1d array"):
            fn(x, lab.reshape(3, 2))
        with pytest.raises(ValueError, match="batch_size"):
            fn(x, lab, batch_size=0)
    with pytest.raises(ValueError, match="limit of 524288"):
        K.silhouette_score(torch.zeros(524289, 1), torch.zeros(524289, dtype=torch.int64))
    # the empty paths of the silhouette variants: the reference's all-zero dict and 0.0 for the new key
    zero = {"clustering_ari": 0.0, "clustering_nmi": 0.0, "clustering_v_measure": 0.0, "clustering_silhouette": 0.0}
    zero_best = {"clustering_best_k": 0.0, "clustering_ari_best": 0.0, "clustering_nmi_best": 0.0, "clustering_v_measure_best": 0.0,
                 "clustering_silhouette_best": 0.0}
    assert K.eval_clustering_silhouette(np.zeros((0, 3)), np.zeros(0)) == zero
    assert K.eval_clustering_multiple_k_silhouette(np.zeros((0, 3)), np.zeros(0)) == zero_best
    assert K.eval_clustering_multiple_k_silhouette(x[:4], np.arange(4), k_range=(4, 9)) == zero_best
    with pytest.raises(ValueError, match=r"^Embeddings and labels must have same length: 6 vs 5$"):
        K.eval_clustering_silhouette(x, lab[:5])
    assert set(K.eval_clustering(np.zeros((0, 3)), np.zeros(0))) == {"clustering_ari", "clustering_nmi", "clustering_v_measure"}


def test_label_count_text_is_scikit_learns():
    """The number of distinct labels must be in [2, N - 1]; the check needs the densified ids, so on a machine without a GPU only the
    restatement and scikit-learn are compared here, and the device module in tests/test_gpu_silhouette.py."""
    metrics = pytest.importorskip("sklearn.metrics")
    x = np.random.default_rng(0).standard_normal((6, 3)).astype(np.float32)
    for lab in (np.zeros(6, dtype=int), np.arange(6)):
        with pytest.raises(ValueError) as mine:
            SR.silhouette_samples(x, lab)
        with pytest.raises(ValueError) as theirs:
            metrics.silhouette_samples(x, lab)
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError) as theirs:
        metrics.silhouette_samples(x, np.zeros(5, dtype=int))
    assert str(theirs.value) == "Found input variables with inconsistent numbers of samples: [6, 5]"


def test_layout_of_the_cluster_ordered_rows():
    """_sil_layout on the host: stable inside a cluster, clusters padded to 32 slots, the whole to 128."""
    ids = torch.tensor([2, 0, 1, 0, 2, 2, 0], dtype=torch.int32)
    slot_src, group, counts, n_slots = K._sil_layout(ids, 3, torch.device("cpu"))
    assert n_slots == 128 and counts.tolist() == [3, 1, 3] and group.tolist() == [0, 1, 2, -1]
    s = slot_src.tolist()
    assert s[0:3] == [1, 3, 6] and s[32:33] == [2] and s[64:67] == [0, 4, 5]
    assert sorted(v for v in s if v >= 0) == list(range(7)) and s.count(-1) == 121
    ids = torch.from_numpy(np.repeat(np.arange(3), [33, 64, 1]).astype(np.int32))
    slot_src, group, counts, n_slots = K._sil_layout(ids, 3, torch.device("cpu"))
    assert n_slots == 256 and group.tolist() == [0, 0, 1, 1, 2, -1, -1, -1]


def test_silhouette_args_layout_matches_header(tmp_path):
    import ctypes as C
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _capi.SilhouetteArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/avexhip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(avexhip_silhouette_args));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(avexhip_silhouette_args, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


def test_library_exports_the_silhouette_entry_points(built_lib):
    assert _capi.header_abi_version() >= 12
    for name in ("avexhip_silhouette_workspace_bytes", "avexhip_silhouette_max_labels", "avexhip_silhouette_max_n", "avexhip_silhouette_prepare",
                 "avexhip_silhouette_batch", "avexhip_silhouette_finalize", "avexhip_clustering_centred_rows"):
        assert hasattr(built_lib, name), name
    assert built_lib.avexhip_silhouette_max_labels() == K.MAX_SIL_LABELS >= built_lib.avexhip_clustering_max_k()
    assert built_lib.avexhip_silhouette_max_n() == K.MAX_SIL_N
    # O(N D + batch n_labels): the ordered rows, one norm per slot, one 64-bit sum per (batch row, cluster) -- no N x N matrix
    n, d, k, batch = 65536, 768, 512, 2048
    n_slots = n + 32 * k
    ws = built_lib.avexhip_silhouette_workspace_bytes(n_slots, d, k, batch)
    assert n_slots * d * 4 <= ws <= n_slots * d * 4 + n_slots * 4 + batch * k * 8 + (1 << 16)
    assert ws < n * n * 4
    assert built_lib.avexhip_silhouette_workspace_bytes(n_slots, d, 4097, batch) == 0
    assert built_lib.avexhip_silhouette_workspace_bytes(0, d, k, batch) == 0
    assert built_lib.avexhip_silhouette_workspace_bytes(524288 + 32 * 4096 + 128, d, 4096, batch) > 0
    assert built_lib.avexhip_clustering_centred_rows(None) is None


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x, lab = SR.case_inputs("c300")
    with pytest.raises(_capi.AvexHipError):
        K.silhouette_score(x, lab)
    with pytest.raises(_capi.AvexHipError):
        K.silhouette_samples(x, lab, metric="cosine")
    with pytest.raises(_capi.AvexHipError):
        K.eval_clustering_silhouette(x, lab)
