"""avex_amd.retrieval without a GPU: the NumPy restatement (tests/_retrieval_ref.py) against the real reference's outputs
(tests/golden/retrieval.npz, written by tests/golden/make_retrieval_goldens.py), and the public module's contract -- signatures,
defaults, ValueError texts, label reductions, the C struct mirror."""
import inspect
import os

import numpy as np
import pytest
import torch

import _retrieval_ref as RR
from avex_amd import _capi
from avex_amd import retrieval as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["evaluate_auc_roc", "evaluate_auc_roc_batched", "evaluate_auc_roc_cross_set", "evaluate_precision", "evaluate_precision_batched",
          "evaluate_precision_cross_set", "eval_retrieval", "eval_retrieval_cross_set"]
# names, defaults of the reference's signatures (avex/evaluation/retrieval.py), for machines where it cannot be imported
SIGNATURES = {
    "evaluate_auc_roc": [("embeddings", None), ("labels", None)],
    "evaluate_auc_roc_batched": [("embeddings", None), ("labels", None), ("batch_size", 2048)],
    "evaluate_auc_roc_cross_set": [("query_embeds", None), ("query_labels", None), ("db_embeds", None), ("db_labels", None)],
    "evaluate_precision": [("embeddings", None), ("labels", None), ("k", 1)],
    "evaluate_precision_batched": [("embeddings", None), ("labels", None), ("k", 1), ("batch_size", 2048)],
    "evaluate_precision_cross_set": [("query_embeds", None), ("query_labels", None), ("db_embeds", None), ("db_labels", None), ("k", 1)],
    "eval_retrieval": [("embeds", None), ("labels", None), ("batch_size", 2048)],
    "eval_retrieval_cross_set": [("query_embeds", None), ("query_labels", None), ("db_embeds", None), ("db_labels", None)],
}


def _sig(fn):
    return [(n, None if p.default is inspect.Parameter.empty else p.default) for n, p in inspect.signature(fn).parameters.items()]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return RR.load_golden(golden_dir)


def _case_names(meta, self_set):
    return [n for n, c in meta["cases"].items() if c["self_set"] == self_set]


def test_golden_covers_the_cases(golden):
    z, meta = golden
    assert set(meta["cases"]) >= {"hard", "easy_d768", "onehot2d", "multihot80", "singleton", "zero_row", "dup_rows", "cross_ids",
                                  "cross_allpos", "cross_mix", "cross_1d_db"}
    assert 0.5 < meta["cases"]["hard"]["auc"] < 0.6                                    # hard: an easy set hides errors
    assert z["multihot80/labels"].shape[1] > 64
    assert np.isnan(z["singleton/auc_per_query"]).sum() == 2                           # the single-member classes are skipped
    assert np.isnan(z["cross_allpos/auc_per_query"])[0]                                # every database item positive: skipped
    assert np.abs(z["zero_row/x"][5]).max() == 0
    for name, c in meta["cases"].items():
        assert max(c["excluded_share"].values()) <= meta["max_excluded"], name


def test_numpy_restatement_matches_reference_means(golden):
    """Mean metrics within 1e-12 of the reference's (fp64 inputs), every case, k in {1, 5, 10}."""
    z, meta = golden
    for name in _case_names(meta, True):
        c = meta["cases"][name]
        x, lab = z[f"{name}/x"].astype(np.float64), z[f"{name}/labels"]
        for k in meta["ks"]:
            auc, prec = RR.metrics_from_stats(RR.self_stats(x, lab, k))
            assert abs(auc - c["auc"]) <= 1e-12, (name, auc, c["auc"])
            # the reference's batched product (100 x N blocks) rounds a duplicated row's similarities differently from block to block, so
            # its exact ties stop being ties (4e-7 on the mean, reference against itself); every other case agrees to 1e-12
            assert abs(auc - c["auc_batched"]) <= (1e-6 if name == "dup_rows" else 1e-12), (name, auc, c["auc_batched"])
            if name in ("dup_rows", "zero_row") and k > 1:
                continue      # exact ties at the k-th place: np.argpartition's pick is unspecified
            assert abs(prec - c["precision"][str(k)]) <= 1e-12 and abs(prec - c["precision_batched"][str(k)]) <= 1e-12, (name, k, prec)
        assert abs(c["eval_retrieval"]["retrieval_roc_auc"] - c["auc"]) <= 1e-12
    for name in _case_names(meta, False):
        c = meta["cases"][name]
        q, d = z[f"{name}/q"].astype(np.float64), z[f"{name}/d"].astype(np.float64)
        for k in meta["ks"]:
            auc, prec = RR.metrics_from_stats(RR.cross_stats(q, z[f"{name}/q_labels"], d, z[f"{name}/d_labels"], k))
            assert abs(auc - c["auc_cross"]) <= 1e-12, (name, auc)
            assert abs(prec - c["precision_cross"][str(k)]) <= 1e-12, (name, k, prec)


def test_numpy_restatement_matches_reference_per_query(golden):
    """Per query: who is skipped, U2 as an integer against the reference's per-query roc_auc_score, and the top-k hit counts."""
    z, meta = golden
    for name, c in meta["cases"].items():
        if c["self_set"]:
            x = z[f"{name}/x"].astype(np.float64)
            stats = {k: RR.self_stats(x, z[f"{name}/labels"], k) for k in meta["ks"]}
            sim = np.matmul(RR.normed(x), RR.normed(x).T)
            np.fill_diagonal(sim, -np.inf)
        else:
            q, d = z[f"{name}/q"].astype(np.float64), z[f"{name}/d"].astype(np.float64)
            stats = {k: RR.cross_stats(q, z[f"{name}/q_labels"], d, z[f"{name}/d_labels"], k) for k in meta["ks"]}
            sim = np.matmul(RR.normed(q), RR.normed(d).T)
        st = stats[1]
        ref_auc = z[f"{name}/auc_per_query"]
        assert np.array_equal(~np.isnan(ref_auc), st["valid_auc"]), name
        va = st["valid_auc"]
        want = np.rint(ref_auc[va] * 2.0 * st["n_pos"][va] * st["n_neg"][va]).astype(np.int64)
        assert np.array_equal(st["u2"][va], want), name
        assert np.abs(st["u2"][va] / (2.0 * st["n_pos"][va] * st["n_neg"][va]) - ref_auc[va]).max(initial=0.0) <= 1e-15
        srt = -np.sort(-sim, axis=1)
        for a, k in enumerate(meta["ks"]):
            ref_hits = z[f"{name}/hits_per_query"][a]
            assert np.array_equal(ref_hits >= 0, stats[k]["valid_prec"]), (name, k)
            clear = (srt[:, k - 1] - srt[:, k] >= meta["gap"]) & stats[k]["valid_prec"]
            assert np.array_equal(stats[k]["hits"][clear], ref_hits[clear]), (name, k)


def test_signatures_and_defaults():
    for name in PUBLIC:
        assert _sig(getattr(R, name)) == SIGNATURES[name], name
    p = inspect.signature(R.retrieval_stats).parameters
    assert list(p)[:6] == ["query", "query_labels", "db", "db_labels", "k", "batch_size"]
    assert p["db"].default is None and p["db_labels"].default is None and p["k"].default == 1 and p["batch_size"].default == 2048
    assert p["return_sim"].default is False
    import avex_amd
    assert "retrieval" not in avex_amd.__all__ and not any(n in avex_amd.__all__ for n in PUBLIC)


def test_signatures_against_the_reference():
    path = "/root/reference/avex/evaluation/retrieval.py"
    if not os.path.exists(path):
        pytest.skip("reference checkout not on this machine")
    pytest.importorskip("sklearn")
    import importlib.util
    spec = importlib.util.spec_from_file_location("avex_reference_retrieval_sig", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for name in PUBLIC:
        assert _sig(getattr(R, name)) == _sig(getattr(ref, name)) == SIGNATURES[name], name


def test_value_error_texts():
    x, lab = np.zeros((4, 3)), np.arange(4)
    for fn in (R.evaluate_auc_roc, R.evaluate_auc_roc_batched, R.evaluate_precision, R.evaluate_precision_batched, R.eval_retrieval):
        with pytest.raises(ValueError, match=r"^embeddings must be 2-D \(N, D\)$"):
            fn(np.zeros(4), lab)
        with pytest.raises(ValueError, match=r"^labels length must match number of embeddings$"):
            fn(x, lab[:3])
        with pytest.raises(ValueError, match=r"^labels length must match number of embeddings$"):
            fn(torch.zeros(4, 3), torch.arange(3))
    for fn in (R.evaluate_auc_roc_cross_set, R.evaluate_precision_cross_set, R.eval_retrieval_cross_set):
        with pytest.raises(ValueError, match=r"^embeddings must be 2-D \(N, D\)$"):
            fn(x, lab, np.zeros(4), lab)
        with pytest.raises(ValueError, match=r"^query labels length must match number of query embeddings$"):
            fn(x, lab[:3], x, lab)
        with pytest.raises(ValueError, match=r"^database labels length must match number of database embeddings$"):
            fn(x, lab, x, lab[:2])
    with pytest.raises(ValueError, match="limit of 32"):
        R.retrieval_stats(np.zeros((100, 3)), np.zeros(100, dtype=np.int64), k=33)
    with pytest.raises(ValueError, match="limit of 524288"):
        R.retrieval_stats(np.zeros((2, 3)), np.zeros(2), np.broadcast_to(np.zeros(3), ((1 << 19) + 1, 3)), np.zeros((1 << 19) + 1))
    with pytest.raises(ValueError, match="k must be >= 1"):
        R.retrieval_stats(x, lab, k=0)


def test_degenerate_sizes_need_no_device():
    one = np.ones((1, 3))
    assert R.evaluate_precision(one, np.zeros(1)) == 0.0 and R.evaluate_precision_batched(one, np.zeros(1)) == 0.0
    assert R.evaluate_auc_roc(one, np.zeros(1)) == 0.0
    assert R.evaluate_precision_cross_set(one, np.zeros(1), np.zeros((0, 3)), np.zeros(0)) == 0.0
    assert R.evaluate_auc_roc_cross_set(one, np.zeros(1), np.zeros((0, 3)), np.zeros(0)) == 0.0
    assert R.eval_retrieval(one, np.zeros(1)) == {"retrieval_roc_auc": 0.0, "retrieval_precision_at_1": 0.0}


def test_label_reductions():
    """The three label shapes and the cross-set corners, as the module prepares them for the kernel (host tensors: no GPU needed)."""
    cpu = torch.device("cpu")
    ids = np.array([5, -2, 5, 7], dtype=np.int64)
    kind, q, d = R._relevance(torch.from_numpy(ids), None, cpu)
    assert kind == "ids" and q.dtype == torch.int32 and np.array_equal((q[:, None] == d[None, :]).numpy(), RR.relevance_self(ids))
    onehot = np.eye(8, dtype=np.float32)[[1, 3, 1, 0]]
    kind, q, d = R._relevance(torch.from_numpy(onehot), None, cpu)
    assert kind == "ids" and np.array_equal((q[:, None] == d[None, :]).numpy(), RR.relevance_self(onehot))
    assert R._collapse_one_hot(torch.from_numpy(onehot.astype(bool))).dim() == 2            # only f32 / f64 / i32 / i64 collapse
    assert R._collapse_one_hot(torch.tensor([[1, 1], [1, 0]])).dim() == 2                   # genuine multi-hot stays
    assert R._collapse_one_hot(torch.tensor([[0.5, 0.5], [0.0, 1.0]])).tolist() == [0, 1]   # "sums to exactly 1" is the whole rule
    # cross-set: ids across two sets keep ==; mixed dtypes promote
    kind, q, d = R._relevance(torch.tensor([3, 9]), torch.tensor([9.0, 4.0, 3.0]), cpu)
    assert kind == "ids" and (q[:, None] == d[None, :]).tolist() == [[False, False, True], [True, False, False]]
    # 1-D database under 2-D multi-hot queries: nothing is relevant
    kind, q, d = R._relevance(torch.tensor([[1, 1, 0], [0, 1, 1]]), torch.tensor([0, 1, 2]), cpu)
    assert kind == "ids" and not (q[:, None] == d[None, :]).any()
    # one-hot queries collapse, one-hot database collapses -> ids
    kind, q, d = R._relevance(torch.eye(3)[[0, 2]], torch.eye(3)[[2, 2, 1]], cpu)
    assert kind == "ids" and (q[:, None] == d[None, :]).tolist() == [[False, False, False], [True, True, False]]
    with pytest.raises(ValueError):
        R._relevance(torch.tensor([1, 2]), torch.eye(2), cpu)
    strings, none = R._label_tensors(np.array(["cat", "dog", "cat"]))
    assert strings.tolist() == [0, 1, 0] and none is None
    # string labels across two sets get ONE coding: "dog" finds "dog"
    kind, q, d = R._relevance(*R._label_tensors(np.array(["dog"]), np.array(["cat", "dog"])), cpu)
    assert kind == "ids" and (q[:, None] == d[None, :]).tolist() == [[False, True]]
    kind, q, d = R._relevance(*R._label_tensors(["b", "zz"], ["a", "b", "c", "b"]), cpu)
    assert (q[:, None] == d[None, :]).tolist() == [[False, True, False, True], [False] * 4]
    with pytest.raises(ValueError):
        R._label_tensors(np.array(["a"]), np.array([1, 2]))


def test_retrieval_args_layout_matches_header(tmp_path):
    import ctypes as C
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _capi.RetrievalArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/avexhip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(avexhip_retrieval_args));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(avexhip_retrieval_args, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(out[fname]) == getattr(cls, fname).offset, fname


def test_library_exports_the_retrieval_entry_points(built_lib):
    assert _capi.header_abi_version() >= 10
    assert built_lib.avexhip_retrieval_max_k() == R.MAX_K == 32
    # normalised database + normalised batch + similarities, nothing N x N
    n, d, b = 32768, 768, 2048
    ws = built_lib.avexhip_retrieval_workspace_bytes(n, d, b, 0)
    assert n * d * 4 + b * n * 4 <= ws <= n * d * 4 + b * d * 4 + b * n * 4 + 4096
    assert built_lib.avexhip_retrieval_workspace_bytes(0, d, b, 0) == 0


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_capi.AvexHipError):
        R.evaluate_auc_roc(np.random.default_rng(0).standard_normal((8, 4)), np.arange(8) % 2)
