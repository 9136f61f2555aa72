"""avex_amd.clustering without a GPU: the NumPy restatement (tests/_clustering_ref.py) against the real reference's outputs
(tests/golden/clustering.npz, written by tests/golden/make_clustering_goldens.py), and the public module's contract -- signatures,
defaults, return keys, the ValueError text, the rules that need no device, the random-number protocol, the C struct mirror."""
import inspect
import os

import numpy as np
import pytest
import torch

import _clustering_ref as CR
from avex_amd import _capi
from avex_amd import clustering as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# names and defaults of the reference's signatures (avex/evaluation/clustering.py), for machines where it cannot be imported
SIGNATURES = {
    "eval_clustering": [("embeds", None), ("labels", None), ("n_clusters", None), ("random_state", 42)],
    "eval_clustering_multiple_k": [("embeds", None), ("labels", None), ("k_range", None), ("random_state", 42)],
}
EVAL_KEYS = {"clustering_ari", "clustering_nmi", "clustering_v_measure"}
BEST_KEYS = {"clustering_best_k", "clustering_ari_best", "clustering_nmi_best", "clustering_v_measure_best"}


def _sig(fn):
    return [(n, None if p.default is inspect.Parameter.empty else p.default) for n, p in inspect.signature(fn).parameters.items()]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return CR.load_golden(golden_dir)


def test_golden_covers_the_cases(golden):
    z, meta = golden
    assert set(meta["cases"]) >= {"set8", "set12", "set20_d768", "set30_d100", "set12_k5", "set12_k30", "labels_n1", "multihot", "label_minus1",
                                  "n6_k10", "one_class", "nan_row"}
    assert set(meta["cases_init"]) == {"relocate", "tol_stop"} and meta["multiple_k"]["case"] == "set8"
    assert meta["max_unstable"] == 0 and meta["min_gap"] == 1e-5 and meta["noise"] == 1e-6 and len(meta["noise_seeds"]) == 3
    c = meta["cases"]
    assert (c["set12_k5"]["k"], c["set12_k30"]["k"], c["set12"]["k"]) == (5, 30, 12)
    assert c["set30_d100"]["gen"]["d"] == 100 and c["set30_d100"]["gen"]["n"] % 128 != 0
    assert z["labels_n1/labels"].ndim == 2 and z["labels_n1/labels"].shape[1] == 1
    assert z["multihot/labels"].shape[1] == 6 and (z["multihot/labels"].sum(axis=1) > 1).any()
    assert (z["label_minus1/labels"] == -1).any() and c["label_minus1"]["k"] == 5
    assert c["n6_k10"]["n_clusters"] == 10 and c["n6_k10"]["k"] == 6
    assert c["one_class"]["eval_clustering"] == CR.ZERO and c["nan_row"]["eval_clustering"] == CR.ZERO
    assert np.isnan(z["nan_row/x"]).any()
    for name, m in c.items():
        gap = m.get("nearest_other_partition_gap")
        assert gap is None or gap >= meta["min_gap"], name
    assert meta["cases_init"]["relocate"]["strict"] and not meta["cases_init"]["tol_stop"]["strict"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "clustering.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "retrieval.npz"))


def test_restatement_reproduces_the_reference_partition(golden):
    """Every case: the restatement's partition IS the reference's (their ARI is exactly 1.0), n_iter and the first restart's seed rows
    are scikit-learn's, and the three scores are within 1e-12 of the reference's."""
    z, meta = golden
    for name, c in meta["cases"].items():
        x, lab = CR.case_inputs(z, meta, name)
        got = CR.eval_clustering(x, lab, n_clusters=c["n_clusters"])
        ref = c["eval_clustering"]
        for key in EVAL_KEYS:
            assert abs(got[key] - ref[key]) <= 1e-12, (name, key, got[key], ref[key])
        if f"{name}/km_labels" not in z:
            continue
        mine = CR.kmeans(x, c["k"])
        assert CR.scores(mine["labels"], z[f"{name}/km_labels"])[0] == 1.0 and CR.same_partition(mine["labels"], z[f"{name}/km_labels"]), name
        assert mine["n_iter"] == c["n_iter"], name
        assert np.array_equal(mine["seed_indices"][0], z[f"{name}/seeds0"]), name
        assert abs(mine["inertia"] - c["inertia"]) <= 1e-5 * c["inertia"], name
        assert mine["best_init"] == c["restatement_best_init"]


def test_restatement_explicit_init_relocation_and_tolerance(golden):
    z, meta = golden
    for name, c in meta["cases_init"].items():
        info, trace = {}, []
        mine = CR.kmeans(z[f"{name}/x"], c["k"], init=z[f"{name}/init"], tol=c["tol"], trace=trace, info=info)
        assert CR.same_partition(mine["labels"], z[f"{name}/km_labels"]) and mine["n_iter"] == c["n_iter"], name
        assert info["strict"] == c["strict"], name
        if name == "relocate":
            assert (np.bincount(trace[0], minlength=c["k"]) == 0).sum() == 2
            assert np.bincount(mine["labels"], minlength=c["k"]).min() > 0


def test_multiple_k_by_the_restatement(golden):
    z, meta = golden
    mk = meta["multiple_k"]
    x, lab = CR.case_inputs(z, meta, mk["case"])
    best, best_k = -1.0, None
    for k, c in sorted(mk["per_k"].items(), key=lambda kv: int(kv[0])):
        got = CR.eval_clustering(x, lab, n_clusters=int(k))
        for key in EVAL_KEYS:
            assert abs(got[key] - c["eval_clustering"][key]) <= 1e-12, (k, key)
        if got["clustering_ari"] > best:
            best, best_k = got["clustering_ari"], int(k)
    assert float(best_k) == mk["result"]["clustering_best_k"] and abs(best - mk["result"]["clustering_ari_best"]) <= 1e-12
    assert [int(k) for k in mk["per_k"]] == list(range(6, 12))      # max(2, 8 - 2) .. min(N // 2, 8 + 3)


def test_score_formulas_against_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    pairs = [(rng.integers(0, a, size=n), rng.integers(0, b, size=n)) for a, b, n in ((3, 4, 50), (10, 10, 1000), (40, 7, 5000), (2, 2, 7), (200, 150, 3000))]
    t = rng.integers(0, 6, size=400)
    pairs += [(t, (t + rng.integers(0, 2, size=400) * (rng.random(400) < 0.2)) % 6), (t, t), (t, (t * 5 + 1) % 6)]
    pairs += [(np.zeros(4, int), np.ones(4, int)), (np.array([0, 0, 1, 1]), np.full(4, 5)), (np.arange(4), np.arange(4)), (np.zeros(4, int), np.arange(4)),
              (np.array([0, 1, 0, 1]), np.array([0, 0, 1, 1])), (np.array([3]), np.array([9])), (np.array([-1, -1, 2, 2, 7]), np.array([0, 1, 1, 0, 0]))]
    for a, b in pairs:
        got = CR.scores(a, b)
        want = (metrics.adjusted_rand_score(a, b), metrics.normalized_mutual_info_score(a, b), metrics.v_measure_score(a, b))
        assert max(abs(g - w) for g, w in zip(got, want)) <= 1e-12, (a[:8], b[:8], got, want)


# ------------------------------------------------------------------------------------------------------------------------------
#  Past the shapes of clustering.npz (tests/golden/metrics_wide.npz): rows wider than 1024 columns, k above one 128-column assign tile,
#  a contingency table of hundreds x hundreds of classes.  Every input the GPU tests of these shapes use is reproduced here first.
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(golden_dir):
    return CR.load_wide(golden_dir)


def test_wide_golden_covers_the_cases(wide):
    z, meta = wide
    c = meta["cases"]
    assert set(c) == {"wide8_d1280", "wide10_d1536", "set40_k150", "set20_k200"}
    assert meta["max_unstable"] == 0 and meta["min_gap"] == 1e-5 and meta["noise"] == 1e-6 and len(meta["noise_seeds"]) == 3
    assert (c["wide8_d1280"]["gen"]["d"], c["wide10_d1536"]["gen"]["d"]) == (1280, 1536)                  # dpad > 1024: two column blocks
    assert (c["set40_k150"]["k"], c["set20_k200"]["k"]) == (150, 200)                                     # kpad 160 and 224
    assert [K._trials(m["k"]) for m in c.values()] == [4, 4, 7, 7] and 10 * K._trials(150) > 64           # more than 64 seeding candidates
    for name, m in c.items():
        assert m["nearest_other_partition_gap"] is None or m["nearest_other_partition_gap"] >= meta["min_gap"], name
        assert z[f"{name}/km_labels"].shape == (m["gen"]["n"],) and z[f"{name}/seeds0"].shape == (m["k"],)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "metrics_wide.npz")) < 1 << 20


@pytest.mark.parametrize("name", ["wide8_d1280", "wide10_d1536", "set40_k150", "set20_k200"])
def test_restatement_reproduces_the_wide_cases(wide, name):
    """As test_restatement_reproduces_the_reference_partition: scikit-learn's partition, n_iter, first-restart seed rows and inertia, and
    the reference's three scores within 1e-12."""
    z, meta = wide
    c = meta["cases"][name]
    x, lab = CR.case_inputs(z, meta, name)
    mine = CR.kmeans(x, c["k"])
    assert CR.scores(mine["labels"], z[f"{name}/km_labels"])[0] == 1.0 and CR.same_partition(mine["labels"], z[f"{name}/km_labels"])
    assert mine["n_iter"] == c["n_iter"]
    assert np.array_equal(mine["seed_indices"][0], z[f"{name}/seeds0"])
    assert abs(mine["inertia"] - c["inertia"]) <= 1e-5 * c["inertia"]
    assert mine["best_init"] == c["restatement_best_init"]
    sc = CR.scores(CR.reduce_labels(lab), mine["labels"])
    for key, v in zip(("clustering_ari", "clustering_nmi", "clustering_v_measure"), sc):
        assert abs(v - c["eval_clustering"][key]) <= 1e-12, (key, v)


def test_separated_sets_have_a_margin():
    """The condition under which tests/test_gpu_clustering.py asks for label equality with NumPy on EVERY point: in each checked assign
    (from the explicit init and after one and two updates) the fp64 gap between a point's nearest and second-nearest centre is at
    least 1e-4 of the nearest squared distance.  The same for the k = 1100 set from either restart's seed rows, whose restarts' inertias
    are far enough apart that both sides pick the same winner, and for the two relocation sets (bit-identical centres counted once)."""
    for k, seed in {130: 130, 160: 160, 257: 258}.items():
        x, lab = CR.separated(seed, k, 3, 16)
        assert x.shape == (3 * k, 16) and np.bincount(lab).tolist() == [3] * k
        init = x[np.random.default_rng(k).choice(x.shape[0], size=k, replace=False)]
        assert CR.assign_margin(x, init, 3) >= 1e-4, k
    x, _ = CR.separated(7, 1100, 3, 16)
    km = CR.kmeans(x, 1100, n_init=2, max_iter=1)
    assert K._trials(1100) == 9 and km["seed_indices"].shape == (2, 1100)
    assert abs(km["inertias"][0] - km["inertias"][1]) >= 1e-4 * km["inertias"].min()
    for r in range(2):
        assert CR.assign_margin(x, x[km["seed_indices"][r]], 2) >= 1e-4, r
    for k, copies, per, d, seed in ((160, 20, 5, 16, 99), (12, 3, 8, 1100, 98)):
        x, _ = CR.separated(seed, k, per, d)
        init = CR.duplicate_init(x, k, copies, 5)
        assert np.unique(init, axis=0).shape[0] == k - copies + 1
        assert CR.assign_margin(x, init, 4) >= 1e-4, k
        trace = []
        CR.kmeans(x, k, init=init, max_iter=3, trace=trace)
        assert (np.bincount(trace[0], minlength=k) == 0).sum() == copies - 1      # the first copy wins every tie; the rest start empty


def test_scores_on_a_large_table(wide):
    """The restatement against sklearn.metrics on a table of 300 x 350 occupied classes: the values the generator recorded, and
    scikit-learn itself where it is installed."""
    _, meta = wide
    rec = meta["scores_table"]
    a, b = CR.label_pair(**rec["gen"])
    assert CR.sha256(a, b) == rec["sha256"] and rec["gen"]["n"] == 20000
    t = CR.contingency(a, b)
    assert t.shape == (300, 350) == (rec["classes_true"], rec["classes_pred"]) and (t > 0).sum() > 5000      # the goldens: at most 30 x 30 cells
    got = CR.scores(a, b)
    assert max(abs(got[0] - rec["ari"]), abs(got[1] - rec["nmi"]), abs(got[2] - rec["v_measure"])) <= 1e-12, (got, rec)
    try:
        from sklearn import metrics
    except ImportError:
        return
    want = (metrics.adjusted_rand_score(a, b), metrics.normalized_mutual_info_score(a, b), metrics.v_measure_score(a, b))
    assert max(abs(g - w) for g, w in zip(got, want)) <= 1e-12, (got, want)


def test_random_number_protocol():
    """The module's draws are the restatement's (which the golden pins to scikit-learn through the seed rows), they depend on (n, k,
    n_init, seed) only, and another seed gives other numbers."""
    for n, k in ((2000, 8), (1500, 30), (6, 6), (50, 2)):
        f1, u1 = K._draws(n, k, 10, 42)
        f2, u2 = CR.draws(n, k, 10, 42)
        assert np.array_equal(f1, f2) and np.array_equal(u1, u2)
        assert u1.shape == (10, k - 1, 2 + int(np.log(k))) and (0 <= f1).all() and (f1 < n).all()
        assert not np.array_equal(K._draws(n, k, 10, 7)[1], u1)
    assert [K._trials(k) for k in (2, 3, 7, 8, 20, 21, 54, 55, 148, 149, 403, 404, 1096, 1097, 2980, 2981, 4096)] == \
        [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10]


def test_signatures_defaults_and_keys():
    for name, sig in SIGNATURES.items():
        assert _sig(getattr(K, name)) == sig, name
    p = inspect.signature(K.kmeans).parameters
    assert list(p)[:2] == ["x", "n_clusters"]
    assert {n: p[n].default for n in ("n_init", "max_iter", "tol", "random_state", "init")} == \
        {"n_init": 10, "max_iter": 300, "tol": 1e-4, "random_state": 42, "init": None}
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("n_init", "max_iter", "tol", "random_state", "init"))
    assert list(inspect.signature(K.clustering_scores).parameters) == ["labels_true", "labels_pred"]
    assert set(K._get_empty_clustering_metrics()) == EVAL_KEYS and set(K._get_empty_clustering_best_metrics()) == BEST_KEYS
    assert K.MAX_K == 4096
    import avex_amd
    assert "clustering" not in avex_amd.__all__


def test_signatures_against_the_reference():
    path = "/root/reference/avex/evaluation/clustering.py"
    if not os.path.exists(path):
        pytest.skip("reference checkout not on this machine")
    pytest.importorskip("sklearn")
    import importlib.util
    spec = importlib.util.spec_from_file_location("avex_reference_clustering_sig", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for name, sig in SIGNATURES.items():
        assert _sig(getattr(K, name)) == _sig(getattr(ref, name)) == sig, name
    assert ref._get_empty_clustering_metrics() == K._get_empty_clustering_metrics()
    assert ref._get_empty_clustering_best_metrics() == K._get_empty_clustering_best_metrics()


def test_rules_that_need_no_device():
    x, lab = np.zeros((4, 3), dtype=np.float32), np.arange(4)
    for fn, zero in ((K.eval_clustering, CR.ZERO), (K.eval_clustering_multiple_k, CR.ZERO_BEST)):
        assert fn(np.zeros((0, 3)), np.zeros(0)) == zero
        assert fn(torch.zeros(0, 3), torch.zeros(0)) == zero
        assert fn(x, np.zeros(0)) == zero
    with pytest.raises(ValueError, match=r"^Embeddings and labels must have same length: 4 vs 3$"):
        K.eval_clustering(x, lab[:3])
    with pytest.raises(ValueError, match=r"^Embeddings and labels must have same length: 4 vs 3$"):
        K.eval_clustering(torch.zeros(4, 3), torch.arange(3))
    with pytest.raises(ValueError, match="limit of 4096"):
        K.kmeans(np.zeros((5000, 2), dtype=np.float32), 4097)
    with pytest.raises(ValueError, match="n_init"):
        K.kmeans(np.zeros((50, 2), dtype=np.float32), 3, n_init=65)
    with pytest.raises(ValueError, match=r"n_samples=4 should be >= n_clusters=5"):
        K.kmeans(x, 5)
    with pytest.raises(ValueError, match="2-D"):
        K.kmeans(np.zeros(4), 2)
    with pytest.raises(ValueError):
        K.clustering_scores(np.arange(4), np.arange(3))
    assert K._reduce_labels(np.arange(5).reshape(5, 1)).tolist() == [0, 1, 2, 3, 4]
    assert K._reduce_labels(np.array([[0, 1, 1], [1, 0, 0], [0, 0, 0]])).tolist() == [1, 0, 0]      # argmax: the first maximum
    assert K.eval_clustering_multiple_k(x, lab, k_range=(4, 9)) == CR.ZERO_BEST                     # stops at k >= N: nothing to try


def test_clustering_args_layout_matches_header(tmp_path):
    import ctypes as C
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _capi.ClusteringArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/avexhip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(avexhip_clustering_args));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(avexhip_clustering_args, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


def test_library_exports_the_clustering_entry_points(built_lib):
    assert _capi.header_abi_version() >= 11
    assert built_lib.avexhip_clustering_max_k() == K.MAX_K
    assert [built_lib.avexhip_clustering_trials(k) for k in (2, 8, 20, 64, 512, 4096)] == [K._trials(k) for k in (2, 8, 20, 64, 512, 4096)]
    # O(N dpad + N R (trials + few) + R k dpad): centred data, per-restart point vectors, two centre tables -- no N x R k matrix
    n, d, k, r = 65536, 768, 512, 10
    ws = built_lib.avexhip_clustering_workspace_bytes(n, d, k, r)
    t = K._trials(k)
    assert n * d * 4 <= ws <= n * d * 4 + n * r * (4 * t + 32) + 2 * r * k * d * 4 + (1 << 20)
    assert ws < n * r * k * 4
    assert built_lib.avexhip_clustering_workspace_bytes(n, d, 4097, r) == 0 and built_lib.avexhip_clustering_workspace_bytes(0, d, k, r) == 0
    # the (n, d) head comes first: a workspace sized for a larger k serves a smaller one
    assert built_lib.avexhip_clustering_workspace_bytes(n, d, 6, r) < built_lib.avexhip_clustering_workspace_bytes(n, d, 11, r) or \
        built_lib.avexhip_clustering_workspace_bytes(n, d, 6, r) == built_lib.avexhip_clustering_workspace_bytes(n, d, 11, r)


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rng = np.random.default_rng(0)
    with pytest.raises(_capi.AvexHipError):
        K.eval_clustering(rng.standard_normal((8, 4)), np.arange(8) % 2)
    with pytest.raises(_capi.AvexHipError):
        K.kmeans(rng.standard_normal((8, 4)), 2)
    with pytest.raises(_capi.AvexHipError):
        K.clustering_scores(np.arange(8) % 2, np.arange(8) % 3)
