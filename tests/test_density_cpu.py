"""avex_amd.density without a GPU: the NumPy restatement (tests/_density_ref.py) against scikit-learn's DBSCAN and against the recorded
goldens, the argument checks, and the bindings of the avexhip_density_* entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _density_ref as D
from avex_amd import _capi, density, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("avexhip_density_workspace_bytes", "avexhip_density_max_block", "avexhip_density_begin", "avexhip_density_norms", "avexhip_density_count",
        "avexhip_density_core", "avexhip_density_round_begin", "avexhip_density_hook", "avexhip_density_round_end", "avexhip_density_labels",
        "avexhip_density_summary")
CASE_IDS = [f"n{n}-d{d}-{m}" for n, d in D.CASES for m in D.METRICS]
CASE_ARGS = [(n, d, m) for n, d in D.CASES for m in D.METRICS]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "density.npz"))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_by_hand():
    """Six points on a line, euclidean, eps 1, min_samples 3: 0-1-2 chained, 3 a border row of them, 5 and 6 far away."""
    x = np.array([[0.0], [1.0], [2.0], [3.0], [10.0], [20.0]], dtype=np.float32)
    r = D.dbscan(x, eps=1.0, min_samples=3, metric="euclidean")
    assert r["n_neighbors"].tolist() == [2, 3, 3, 2, 1, 1] and r["core"].tolist() == [False, True, True, False, False, False]
    assert r["labels"].tolist() == [0, 0, 0, 0, -1, -1] and r["n_clusters"] == 1 and r["sizes"].tolist() == [4] and r["exemplar"].tolist() == [1]
    r = D.dbscan(x, eps=1.0, min_samples=1, metric="euclidean")                            # every row core: components of the graph
    assert r["labels"].tolist() == [0, 0, 0, 0, 1, 2] and r["exemplar"].tolist() == [1, 4, 5]


def test_restatement_border_row_takes_the_lower_cluster():
    """A similarity matrix given by hand: rows 0-2 and 4-6 are two triangles, row 3 is near one row of each: the two core rows."""
    s = np.eye(7, dtype=np.float32)
    for a, b in ((0, 1), (0, 2), (1, 2), (4, 5), (4, 6), (5, 6), (3, 2), (3, 4)):
        s[a, b] = s[b, a] = 0.95
    r = D.dbscan(sim=s, eps=0.1, min_samples=4, metric="cosine")                             # rows 2 and 4 alone have four neighbours
    assert r["core"].tolist() == [False, False, True, False, True, False, False] and r["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1]
    order = [6, 5, 4, 3, 2, 1, 0]                                                            # the other row order: numbers follow the lowest core row
    r = D.dbscan(sim=s[np.ix_(order, order)], eps=0.1, min_samples=4, metric="cosine")
    assert r["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1] and r["sizes"].tolist() == [4, 3]
    assert r["n_neighbors"].tolist() == [3, 3, 4, 3, 4, 3, 3] and r["exemplar"].tolist() == [2, 4]


def test_restatement_rows_outside_the_graph():
    x = np.array([[1, 0], [1, 0], [np.nan, 0], [1, 0], [np.inf, 1], [0, 0]], dtype=np.float32)
    r = D.dbscan(x, eps=0.0, min_samples=3, metric="cosine")
    assert r["nonfinite"] == 2 and r["n_neighbors"].tolist() == [3, 3, 0, 3, 0, 1]          # the zero row is its own neighbour and nobody else's
    assert r["labels"].tolist() == [0, 0, -1, 0, -1, -1] and r["core"].tolist() == [True, True, False, True, False, False]
    r = D.dbscan(x[[0, 1, 3, 5]], eps=0.0, min_samples=9, metric="cosine")
    assert r["n_clusters"] == 0 and (r["labels"] == -1).all() and r["sizes"].shape == (0,) and r["exemplar"].shape == (0,)


@pytest.mark.parametrize("n,d,metric", CASE_ARGS, ids=CASE_IDS)
def test_restatement_equals_sklearn(n, d, metric):
    """Planted clusters, eps in the middle of the widest gap of the pairwise distances near their 5 % quantile: the gap is at least
    3e-5 (cosine) / 4e-4 (euclidean), some 30 times the error of the fp32 distances, so no pair sits at the threshold and the fp32
    restatement must agree with scikit-learn's fp64 DBSCAN on every row."""
    cluster = pytest.importorskip("sklearn.cluster")
    x = D.planted(D.case_name(n, d), n, d)
    eps, gap = D.gap_eps(x, metric)
    assert gap >= D.MIN_GAP[metric], gap
    fit = cluster.DBSCAN(eps=eps, min_samples=D.MIN_SAMPLES, metric=metric, algorithm="brute").fit(x.astype(np.float64))
    mine = D.dbscan(x, eps=eps, min_samples=D.MIN_SAMPLES, metric=metric)
    assert np.array_equal(mine["labels"], fit.labels_.astype(np.int32))
    assert np.array_equal(np.flatnonzero(mine["core"]), np.sort(fit.core_sample_indices_))
    assert mine["nonfinite"] == 0 and mine["n_clusters"] == int(fit.labels_.max()) + 1


@pytest.mark.parametrize("n,d,metric", CASE_ARGS, ids=CASE_IDS)
def test_restatement_equals_the_recorded_goldens(golden, n, d, metric):
    key = f"{D.case_name(n, d)}/{metric}"
    x = D.planted(D.case_name(n, d), n, d)
    eps, gap = D.gap_eps(x, metric)
    assert eps == float(golden[f"{key}/eps"]) and gap >= D.MIN_GAP[metric]                   # the inputs are the recorded ones
    mine = D.dbscan(x, eps=eps, min_samples=D.MIN_SAMPLES, metric=metric)
    assert np.array_equal(mine["labels"], golden[f"{key}/labels"]) and np.array_equal(np.flatnonzero(mine["core"]), golden[f"{key}/core"])


def test_goldens_are_not_trivial(golden):
    several = sum(int(golden[f"{D.case_name(n, d)}/{m}/labels"].max()) + 1 >= 3 for n, d, m in CASE_ARGS)
    noise = sum(int((golden[f"{D.case_name(n, d)}/{m}/labels"] < 0).sum()) > 0 for n, d, m in CASE_ARGS)
    border = 0
    for n, d, m in CASE_ARGS:
        lab, core = golden[f"{D.case_name(n, d)}/{m}/labels"], golden[f"{D.case_name(n, d)}/{m}/core"]
        border += int((lab >= 0).sum()) > len(core)
    assert several >= 12 and noise == len(CASE_ARGS) and border >= 12, (several, noise, border)


def test_k_distance_restatement():
    s = np.array([[1.0, 0.5, 0.25, np.nan], [0.5, 1.0, 0.75, np.nan], [0.25, 0.75, 1.0, np.nan], [np.nan] * 4], dtype=np.float32)
    assert D.k_distance(s, 1).tolist() == [0.5, 0.25, 0.25, np.inf] and D.k_distance(s, 2).tolist() == [0.75, 0.5, 0.75, np.inf]
    assert np.isinf(D.k_distance(s, 3)).all()


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_raise_without_a_gpu():
    x = np.zeros((4, 3), dtype=np.float32)
    for bad in (-1e-3, float("nan"), float("inf"), 1e39, "0.1", None, True):
        with pytest.raises(ValueError, match="eps"):
            density.dbscan(x, bad)
    for bad in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="min_samples"):
            density.dbscan(x, 0.1, bad)
    for bad in ("dot", "l2", None):
        with pytest.raises(ValueError, match="metric"):
            density.dbscan(x, 0.1, metric=bad)
    for bad in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match="batch_size"):
            density.dbscan(x, 0.1, batch_size=bad)
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="max_rounds"):
            density.dbscan(x, 0.1, max_rounds=bad)
    for bad in (np.zeros(3, dtype=np.float32), np.zeros((0, 3), dtype=np.float32), np.zeros((3, 0), dtype=np.float32), np.zeros((2, 2, 2), dtype=np.float32)):
        with pytest.raises(ValueError, match="shape"):
            density.dbscan(bad, 0.1)
    with pytest.raises(ValueError, match="dot"):
        density.dbscan(search.EmbeddingIndex(8, metric="dot"), 0.1)
    with pytest.raises(ValueError, match="euclidean"):
        density.dbscan(search.EmbeddingIndex(8), 0.1, metric="euclidean")
    with pytest.raises(ValueError, match="empty"):
        density.dbscan(search.EmbeddingIndex(8), 0.1)
    with pytest.raises(ValueError, match="EmbeddingIndex"):
        density.k_distance(x, 1)
    with pytest.raises(ValueError, match="dot"):
        density.k_distance(search.EmbeddingIndex(8, metric="dot"), 1)
    for bad in (0, search.MAX_K + 1, 1.0, True):
        with pytest.raises(ValueError, match="k="):
            density.k_distance(search.EmbeddingIndex(8), bad)
    with pytest.raises(ValueError, match="empty"):
        density.k_distance(search.EmbeddingIndex(8), 3)


def test_exported_from_the_package():
    import avex_amd
    assert avex_amd.dbscan is density.dbscan and avex_amd.k_distance is density.k_distance
    for word in ("Prepared rows", "Distance", "Neighbour", "Symmetry", "Counts and core rows", "Clusters", "Independence", "SYNCHRONISES"):
        assert word in density.__doc__, word


# ------------------------------------------------------------------------------------------------------------------ the bindings
def test_bindings(built_lib):
    assert _capi.header_abi_version() >= 20
    for name in SYMS:
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name
    hdr = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/avexhip.h").read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(avexhip_density_[a-z0-9_]+)\s*\(", hdr))) == sorted(SYMS)
    assert built_lib.avexhip_density_max_block() == density.MAX_BLOCK
    assert "density.hip" in __import__("avex_amd.build", fromlist=["SOURCES"]).SOURCES


def test_density_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the ABI 20 struct as gcc sees include/avexhip.h == the ctypes mirror."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cname, cls = "avexhip_density_args", _capi.DensityArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/avexhip.h"', "int main(void){", f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


def test_workspace_is_linear_in_the_rows_and_knows_no_width(built_lib):
    ws = built_lib.avexhip_density_workspace_bytes
    assert len(_capi.SYMBOLS["avexhip_density_workspace_bytes"][1]) == 1                       # n alone: no width, no n^2
    sizes = [ws(n) for n in (1, 2, 127, 128, 129, 65536, 1 << 20, (1 << 31) - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for n in (65536, 1 << 20, (1 << 31) - 1):
        assert 28 * n <= ws(n) <= 29 * n + 16 * 256, (n, ws(n))                               # five 4-byte and one 8-byte word per row, blocks, flags
    for bad in (0, -1, 1 << 31):
        assert ws(bad) == 0, bad


def _args(**kw):
    fake = 1 << 20                                                        # a 16-byte aligned number: never dereferenced, the call is refused first
    a = _capi.DensityArgs()
    a.n, a.dpad, a.metric, a.eps, a.min_samples = 300, 64, 1, 0.1, 5
    a.rows, a.row0, a.n_rows, a.cols, a.col0, a.n_cols = fake, 0, 300, fake, 0, 300
    a.workspace, a.workspace_bytes = fake, 1 << 30
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def test_entry_points_refuse_bad_shapes(built_lib):
    """rc -1 (-4 for the workspace) and a message that names the offending number, before the device is touched."""
    lib, fake = built_lib, 1 << 20

    def refused(rc, *words, code=-1):
        msg = _capi.last_error()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    every = {"begin": lib.avexhip_density_begin, "norms": lib.avexhip_density_norms, "count": lib.avexhip_density_count, "core": lib.avexhip_density_core,
             "round_begin": lib.avexhip_density_round_begin, "hook": lib.avexhip_density_hook}
    for name, fn in every.items():
        refused(fn(None, None), f"density_{name}", "null")
        refused(fn(C.byref(_args(workspace=None)), None), "null")
        refused(fn(C.byref(_args(n=0)), None), "n 0")
        refused(fn(C.byref(_args(n=1 << 31)), None), str(1 << 31))
        refused(fn(C.byref(_args(dpad=40)), None), "dpad 40")
        refused(fn(C.byref(_args(dpad=0)), None), "dpad 0")
        refused(fn(C.byref(_args(metric=2)), None), "metric 2")
        refused(fn(C.byref(_args(workspace_bytes=1000)), None), "1000", code=-4)
    for name in ("norms", "count", "hook"):
        fn = every[name]
        refused(fn(C.byref(_args(rows=None)), None), "row block")
        refused(fn(C.byref(_args(n_rows=0)), None), "+0")
        refused(fn(C.byref(_args(row0=1)), None), "[1, +300)")
        refused(fn(C.byref(_args(row0=-1, n_rows=10)), None), "[-1, +10)")
        refused(fn(C.byref(_args(n=1 << 23, n_rows=(1 << 22) + 1)), None), str((1 << 22) + 1))
    for name in ("count", "hook"):
        fn = every[name]
        refused(fn(C.byref(_args(cols=None)), None), "column block")
        refused(fn(C.byref(_args(col0=200, n_cols=101)), None), "[200, +101)")
        refused(fn(C.byref(_args(eps=-0.5)), None), "eps -0.5")
        refused(fn(C.byref(_args(eps=float("nan"))), None), "eps")
        refused(fn(C.byref(_args(eps=float("inf"))), None), "eps")
    refused(lib.avexhip_density_core(C.byref(_args(min_samples=0)), None), "min_samples 0")
    refused(lib.avexhip_density_round_end(C.byref(_args()), None, None), "density_round_end", "null")
    refused(lib.avexhip_density_labels(C.byref(_args()), fake, fake, None, fake, None), "density_labels", "null")
    refused(lib.avexhip_density_summary(C.byref(_args()), fake, 0, fake, fake, None), "n_clusters 0")
    refused(lib.avexhip_density_summary(C.byref(_args()), fake, 301, fake, fake, None), "n_clusters 301")
    refused(lib.avexhip_density_summary(C.byref(_args()), None, 3, fake, fake, None), "null")
