"""avex_amd.retrieval on the device against the real reference's outputs (tests/golden/retrieval.npz) and against a NumPy recomputation
from the device's own similarities (tests/_retrieval_ref.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _retrieval_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return RR.load_golden(golden_dir)


@pytest.fixture(scope="module")
def R(built_lib):
    from avex_amd import retrieval
    return retrieval


def _inputs(z, meta, name, dtype=np.float64):
    """(query, query_labels, db, db_labels) of a case; db is None for the self-set ones."""
    if meta["cases"][name]["self_set"]:
        return z[f"{name}/x"].astype(dtype), z[f"{name}/labels"], None, None
    return z[f"{name}/q"].astype(dtype), z[f"{name}/q_labels"], z[f"{name}/d"].astype(dtype), z[f"{name}/d_labels"]


def _relevance(ql, dl):
    return RR.relevance_self(ql) if dl is None else RR.relevance_cross(ql, dl)


def _sim64(q, d):
    return np.matmul(RR.normed(q), RR.normed(q if d is None else d).T)


def test_rank_stage_is_exact_for_the_device_similarities(R, golden):
    """Property check: U2, P, Q, the skip flags and the top-k recomputed in NumPy from the similarity matrix the device itself produced,
    integer for integer, for every query of every golden case, batch sizes that do not divide N and k in {1, 5, 10, 32}."""
    z, meta = golden
    for name in meta["cases"]:
        q, ql, d, dl = _inputs(z, meta, name)
        rel = _relevance(ql, dl)
        base_sim = None
        for k in (1, 5, 10, 32):
            want = None
            for bs in (2048, 100, 1):
                got = R.retrieval_stats(q, ql, d, dl, k=k, batch_size=bs, return_sim=True)
                sim = got["sim"].cpu().numpy()
                if base_sim is None:
                    base_sim = sim
                assert np.array_equal(sim, base_sim), (name, k, bs)      # a similarity does not depend on its batch
                if want is None:
                    want = RR.stats_from_sim(sim, rel, d is None, k)
                assert got["k"] == want["k"]
                for key in ("u2", "n_pos", "n_neg", "valid_auc", "valid_prec", "topk_idx", "hits"):
                    assert np.array_equal(got[key].cpu().numpy(), want[key]), (name, k, bs, key)
                auc, prec = RR.metrics_from_stats(want)
                assert abs(got["auc_sum"] / max(got["auc_count"], 1) - auc) <= 1e-13, (name, k, bs)
                assert abs(got["prec_sum"] / max(got["prec_count"], 1) - prec) <= 1e-13, (name, k, bs)
                assert got["auc_count"] == int(want["valid_auc"].sum()) and got["prec_count"] == int(want["valid_prec"].sum())


def test_similarity_error_against_fp64(R, golden):
    """max |device - fp64| over the matrix, at most 4 x the error of the reference's own fp32 NumPy product on the same inputs (recorded
    by the generator; the margin covers a different summation order)."""
    z, meta = golden
    for name, c in meta["cases"].items():
        q, ql, d, dl = _inputs(z, meta, name)
        sim = R.retrieval_stats(q, ql, d, dl, return_sim=True)["sim"].cpu().numpy().astype(np.float64)
        err = float(np.abs(sim - _sim64(q, d)).max())
        print(f"[retrieval] {name}: similarity max abs error {err:.3e} (reference fp32 {c['ref_fp32_sim_err']:.3e})")
        assert err <= 4.0 * c["ref_fp32_sim_err"], (name, err, c["ref_fp32_sim_err"])


def test_mean_auc_against_the_reference(R, golden):
    """Mean ROC-AUC within 1e-7 of the reference's fp64 value, every case.  The generator records, for the committed `hard` inputs, what
    the reference itself moves by between fp32 and fp64 (3.7e-8: above the 2e-8 expected of a larger set, reported, nothing lowered) and what
    f16-rounded operands would cost (6.6e-8); both are printed.  At N = 1024 -- what fits a committed file -- the 1e-7 bound therefore does
    NOT separate an fp32-class product from an f16 one; test_similarity_error_against_fp64 is the check that does (f16 operands err by
    up to 4.2e-4 in a similarity of this set, 150 x its bound)."""
    z, meta = golden
    hard = meta["cases"]["hard"]
    print(f"[retrieval] hard: reference fp32-vs-fp64 mean AUC spread {abs(hard['auc_fp32'] - hard['auc']):.3e}, "
          f"f16 operands {abs(hard['auc_f16_operands'] - hard['auc']):.3e}")
    for name, c in meta["cases"].items():
        q, ql, d, dl = _inputs(z, meta, name)
        if c["self_set"]:
            got = [R.evaluate_auc_roc(q, ql), R.evaluate_auc_roc_batched(q, ql, batch_size=100), R.eval_retrieval(q, ql)["retrieval_roc_auc"],
                   R.eval_retrieval(torch.from_numpy(q), torch.from_numpy(ql), batch_size=77)["retrieval_roc_auc"]]
            ref = c["auc"]
        else:
            got = [R.evaluate_auc_roc_cross_set(q, ql, d, dl), R.eval_retrieval_cross_set(q, ql, d, dl)["retrieval_roc_auc"]]
            ref = c["auc_cross"]
        print(f"[retrieval] {name}: mean AUC {got[0]!r} reference {ref!r} delta {got[0] - ref:.3e}")
        assert all(g == got[0] for g in got), (name, got)      # batching and the wrapper change nothing
        assert abs(got[0] - ref) <= 1e-7, (name, got[0], ref)
        assert isinstance(got[0], float)


def test_precision_at_k_per_query_against_the_reference(R, golden):
    """Hits in the top k equal to the reference's for every query whose fp64 gap between the k-th and (k+1)-th similarity is at least
    1e-5 (about 50 x the fp32 similarity error); at most 2 % of a case's queries may be left out."""
    z, meta = golden
    for name, c in meta["cases"].items():
        q, ql, d, dl = _inputs(z, meta, name)
        sim = _sim64(q, d)
        if d is None:
            np.fill_diagonal(sim, -np.inf)
        srt = -np.sort(-sim, axis=1)
        for a, k in enumerate(meta["ks"]):
            got = R.retrieval_stats(q, ql, d, dl, k=k)
            ref_hits = z[f"{name}/hits_per_query"][a]
            valid = got["valid_prec"].cpu().numpy()
            assert np.array_equal(valid, ref_hits >= 0), (name, k)
            unclear = srt[:, k - 1] - srt[:, k] < meta["gap"]
            assert unclear.mean() <= 0.02, (name, k, unclear.mean())
            keep = valid & ~unclear
            assert np.array_equal(got["hits"].cpu().numpy()[keep], ref_hits[keep]), (name, k)
            # the public mean: the left-out queries can move it by at most their share
            mean = (R.evaluate_precision_batched(q, ql, k=k, batch_size=100) if d is None else R.evaluate_precision_cross_set(q, ql, d, dl, k=k))
            ref = (c["precision"] if d is None else c["precision_cross"])[str(k)]
            assert abs(mean - ref) <= (unclear & valid).sum() / max(valid.sum(), 1) + 1e-12, (name, k, mean, ref)
            if d is None and k == 1:
                assert R.evaluate_precision(q, ql) == mean == R.eval_retrieval(q, ql)["retrieval_precision_at_1"]


def test_device_resident_input_streams_and_reproducibility(R, golden):
    z, meta = golden
    for name in ("hard", "multihot80", "cross_mix"):
        q, ql, d, dl = _inputs(z, meta, name, np.float32)
        host = R.retrieval_stats(q, ql, d, dl, k=5, return_sim=True)
        dev_args = [None if a is None else torch.from_numpy(a).cuda() for a in (q, ql, d, dl)]
        dev = R.retrieval_stats(*dev_args, k=5, return_sim=True)
        again = R.retrieval_stats(*dev_args, k=5, return_sim=True)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            side = R.retrieval_stats(*dev_args, k=5, return_sim=True)
        stream.synchronize()
        for other in (dev, again, side):
            for key in ("sim", "u2", "n_pos", "n_neg", "topk_idx", "hits", "valid_auc", "valid_prec"):
                assert torch.equal(host[key], other[key]), (name, key)
            assert (host["auc_sum"], host["auc_count"], host["prec_sum"], host["prec_count"]) == \
                   (other["auc_sum"], other["auc_count"], other["prec_sum"], other["prec_count"]), name
        assert dev["u2"].is_cuda and dev["u2"].dtype == torch.int64
    # fp64 on the device is computed in fp32: same bits as the fp32 copy of the same (f16-exact) numbers
    q, ql, _, _ = _inputs(z, meta, "hard", np.float64)
    a = R.retrieval_stats(torch.from_numpy(q).cuda(), torch.from_numpy(ql).cuda())
    b = R.retrieval_stats(q.astype(np.float32), ql)
    assert torch.equal(a["u2"], b["u2"])


def test_string_labels_across_sets_and_separate_stages(R, golden):
    z, meta = golden
    q, ql, d, dl = _inputs(z, meta, "cross_ids")
    names = np.array([f"class{i}" for i in range(200)])
    assert R.evaluate_auc_roc_cross_set(q, names[ql], d, names[dl]) == R.evaluate_auc_roc_cross_set(q, ql, d, dl)
    assert R.evaluate_precision_cross_set(q, list(names[ql]), d, list(names[dl]), k=5) == R.evaluate_precision_cross_set(q, ql, d, dl, k=5)
    # the similarity and the rank stage launched separately (what scripts/retrieval_bench.py times) give the same integers
    x, lab, _, _ = _inputs(z, meta, "hard")
    split = {}
    a, b = R.retrieval_stats(x, lab, k=5, batch_size=300), R.retrieval_stats(x, lab, k=5, batch_size=300, _timing=split)
    assert torch.equal(a["u2"], b["u2"]) and torch.equal(a["topk_idx"], b["topk_idx"]) and a["auc_sum"] == b["auc_sum"]
    assert split["similarity_s"] > 0 and split["rank_s"] > 0


def test_k_above_the_kernel_limit_raises(R):
    x = np.random.default_rng(0).standard_normal((64, 8))
    with pytest.raises(ValueError, match="limit of 32"):
        R.evaluate_precision(x, np.arange(64) % 4, k=33)
    assert 0.0 <= R.evaluate_precision(x[:20], np.arange(20) % 4, k=1000) <= 1.0      # clipped to n - 1 = 19 first, as in the reference
    # cross-set, k == n_db > 1: every database item comes back (the reference raises inside argpartition)
    lab = np.arange(20) % 4
    assert R.evaluate_precision_cross_set(x[:5], lab[:5], x[5:20], lab[5:20], k=15) == pytest.approx(
        np.mean([(lab[5:20] == lab[i]).mean() for i in range(5)]), abs=1e-15)


_MEMORY_CHILD = r"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from avex_amd import retrieval as R
n, d, batch = 32768, 768, 2048
g = torch.Generator(device="cuda").manual_seed(1)
lab = torch.randint(0, 50, (n,), device="cuda", generator=g)
x = torch.randn(n, d, device="cuda", generator=g) + 0.3 * torch.randn(50, d, device="cuda", generator=g)[lab]
R.eval_retrieval(x[:256], lab[:256])                       # library load, kernel attributes
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
before = torch.cuda.memory_allocated()
t0 = time.perf_counter()
out = R.eval_retrieval(x, lab, batch_size=batch)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(json.dumps({"growth": torch.cuda.max_memory_allocated() - before, "inputs": x.numel() * 4 + lab.numel() * 8,
                  "budget": 3 * batch * n * 4, "seconds": dt, "out": out}))
"""


def test_working_memory_is_batch_by_n(R):
    """N = 32768, D = 768, batch 2048: peak device memory grows by no more than inputs + 3 x batch x N x 4 B -- no N x N buffer (4 GiB
    here) -- and the run finishes under its own timeout; no speed bar beyond that."""
    r = subprocess.run([sys.executable, "-c", _MEMORY_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[retrieval] N=32768 D=768: {m['seconds']:.3f} s, peak growth {m['growth'] / 2**20:.0f} MiB (budget {(m['inputs'] + m['budget']) / 2**20:.0f} MiB) {m['out']}")
    assert m["growth"] <= m["inputs"] + m["budget"], m
    assert 0.5 < m["out"]["retrieval_roc_auc"] <= 1.0 and 0.0 <= m["out"]["retrieval_precision_at_1"] <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
#  retr_rank_kernel, chunked U2: the smaller of {positives, negatives} of a query exceeds cap = 16 384 keys, so the kernel sorts it in
#  column chunks of 16 384 (n_db = 40 001: three chunks, the last one 7 233 columns wide -- odd, no multiple of 64).  Per chunk it refills
#  `keys`, resets `fill`, pads with +inf up to the next power of two and skips a chunk without keys.  RR.chunked_case puts into ONE launch
#  queries with pos_small true (class 0: 48 % of the database) and false (class 1: 52 %), a row sorted as a single chunk (class 2: 30
#  items) and a skipped row (class 3: P = 0); every database row exists four times, so equal
#  similarities lie in different chunks and on both sides.  No golden: the reference is NumPy on the device's own similarities.
# ------------------------------------------------------------------------------------------------------------------------------
_INT_KEYS = ("u2", "n_pos", "n_neg", "valid_auc", "valid_prec", "topk_idx", "hits")


def _assert_rank_stage(got, want, tag):
    assert got["k"] == want["k"], tag
    for key in _INT_KEYS:
        g = got[key].cpu().numpy()
        assert np.array_equal(g, want[key]), (tag, key, np.flatnonzero((g != want[key]).reshape(g.shape[0], -1).any(axis=1))[:8])
    auc, prec = RR.metrics_from_stats(want)
    assert abs(got["auc_sum"] / max(got["auc_count"], 1) - auc) <= 1e-13, tag
    assert abs(got["prec_sum"] / max(got["prec_count"], 1) - prec) <= 1e-13, tag
    assert got["auc_count"] == int(want["valid_auc"].sum()) and got["prec_count"] == int(want["valid_prec"].sum()), tag


def test_chunked_rank_path_is_exact_for_the_device_similarities(R):
    """Enters retr_rank_kernel's chunk loop with three chunks, pos_small in both senses, ties across chunk boundaries and a ragged last
    chunk; class ids and, once, multi-hot labels of 70 classes (n_words = 2) through the same chunks.  U2, P, Q, the skip flags, the
    top-k and the hits equal NumPy's on the device's own similarities, integer for integer, k in {1, 32}; the similarities meet the
    bound of test_similarity_error_against_fp64 with the fp32 NumPy product of the same inputs as the yardstick."""
    q, qi, db, di = RR.chunked_case()
    assert db.shape == (40001, 40) and np.unique(db, axis=0).shape[0] == 10001
    counts = np.bincount(di, minlength=4)
    assert min(counts[0], counts[1]) > 16384 and counts[2] == 30 and counts[3] == 0      # both large classes chunk, whichever side is smaller
    rel = RR.relevance_cross(qi, di)
    want, base_sim = {}, None
    for k in (1, 32):
        got = R.retrieval_stats(q, qi, db, di, k=k, return_sim=True)
        sim = got["sim"].cpu().numpy()
        if base_sim is None:
            base_sim = sim
            row = np.sort(sim[0])
            assert (row[1:] == row[:-1]).sum() >= 30000      # the copies of a row really tie, on the device too
        assert np.array_equal(sim, base_sim)
        want[k] = RR.stats_from_sim(sim, rel, False, k)
        _assert_rank_stage(got, want[k], ("ids", k))
    w = want[32]
    assert (w["n_pos"][qi == 0] < w["n_neg"][qi == 0]).all() and (w["n_pos"][qi == 1] > w["n_neg"][qi == 1]).all()      # pos_small true / false
    assert (w["n_pos"][qi == 2] == 30).all() and (w["n_pos"][qi == 3] == 0).all() and not w["valid_auc"][qi == 3].any()
    sim64 = np.matmul(RR.normed(q.astype(np.float64)), RR.normed(db.astype(np.float64)).T)
    ref_err = float(np.abs(np.matmul(RR.normed(q), RR.normed(db).T).astype(np.float64) - sim64).max())
    err = float(np.abs(base_sim.astype(np.float64) - sim64).max())
    print(f"[retrieval] chunked n_db=40001 D=40: similarity max abs error {err:.3e} (NumPy fp32 {ref_err:.3e}, bar {4.0 * ref_err:.3e})")
    assert err <= 4.0 * ref_err, (err, ref_err)
    # the same relevance as two label words per row
    mq, md = RR.multihot_of(qi, 68), RR.multihot_of(di, 69)
    assert RR.collapse_one_hot(mq).ndim == 2 and RR.collapse_one_hot(md).ndim == 2 and np.array_equal(RR.relevance_cross(mq, md), rel)
    got = R.retrieval_stats(q, mq, db, md, k=32, return_sim=True)
    assert np.array_equal(got["sim"].cpu().numpy(), base_sim)
    _assert_rank_stage(got, want[32], ("words", 32))


@pytest.mark.parametrize("n0", [16384, 16385])
def test_chunked_rank_path_at_the_chunk_threshold(R, n0):
    """The balanced class has exactly cap = 16 384 members (the last size sorted as one chunk: cw = the whole row) and 16 385 (the first
    size sorted in chunks of 16 384 columns); the class-1 queries of both variants chunk with pos_small false."""
    q, qi, db, di = RR.chunked_case(n0=n0, per_class=4)
    assert np.bincount(di, minlength=4).tolist() == [n0, 40001 - n0 - 30, 30, 0]
    rel = RR.relevance_cross(qi, di)
    for k in (1, 32):
        got = R.retrieval_stats(q, qi, db, di, k=k, return_sim=True)
        want = RR.stats_from_sim(got["sim"].cpu().numpy(), rel, False, k)
        assert (want["n_pos"][qi == 0] == n0).all() and (want["n_neg"][qi == 0] > n0).all()
        _assert_rank_stage(got, want, (n0, k))


def test_chunked_rank_path_self_set_through_the_c_entry(R, built_lib):
    """Self-set rows of the 40 001-item database, 32 per launch, through avexhip_retrieval_prepare / avexhip_retrieval_batch as
    retrieval_stats drives them (all 40 001 queries would need a 6 GB similarity matrix): q0 puts the column the rank kernel leaves out
    at the end of chunk 0, at the start of chunk 1, across the boundary of chunks 1 and 2, and in the ragged last chunk."""
    import ctypes as C
    from avex_amd import _capi
    _, _, db, di = RR.chunked_case()
    n_db, d, nb, k = db.shape[0], db.shape[1], 32, 32
    x = torch.from_numpy(db).cuda()
    ids = torch.from_numpy(di.astype(np.int32)).cuda()
    lib = built_lib
    ws_bytes = int(lib.avexhip_retrieval_workspace_bytes(n_db, d, nb, 0))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.avexhip_retrieval_prepare(x.data_ptr(), x.stride(0), n_db, d, nb, ws.data_ptr(), ws_bytes, s), "retrieval_prepare")
    for q0 in (16352, 16384, 32752, 39969):
        u2 = torch.empty((nb,), dtype=torch.int64, device="cuda")
        stats = torch.empty((nb, 4), dtype=torch.int32, device="cuda")
        topk = torch.empty((nb, R.MAX_K), dtype=torch.int32, device="cuda")
        sim = torch.empty((nb, n_db), dtype=torch.float32, device="cuda")
        a = _capi.RetrievalArgs()
        a.n_db, a.d, a.batch, a.n_words, a.self_set, a.k, a.stages = n_db, d, nb, 0, 1, k, 3
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        a.db_ids, a.db_words, a.query_words = ids.data_ptr(), None, None
        a.nb, a.q0, a.query, a.ld_query = nb, q0, None, 0
        a.query_ids = ids.data_ptr() + 4 * q0
        a.u2, a.stats, a.topk = u2.data_ptr(), stats.data_ptr(), topk.data_ptr()
        a.sim_out, a.ld_sim = sim.data_ptr(), n_db
        _capi.check(lib.avexhip_retrieval_batch(C.byref(a), s), "retrieval_batch")
        torch.cuda.synchronize()
        rel = di[q0:q0 + nb, None] == di[None, :]
        want = RR.stats_from_sim(sim.cpu().numpy(), rel, True, k, row0=q0)
        st = stats.cpu().numpy()
        assert (np.minimum(want["n_pos"], want["n_neg"])[di[q0:q0 + nb] < 2] > 16384).all()      # these rows chunk
        assert np.array_equal(u2.cpu().numpy(), want["u2"]), (q0, np.flatnonzero(u2.cpu().numpy() != want["u2"]))
        assert np.array_equal(st[:, 0], want["n_pos"]) and np.array_equal(st[:, 1], want["n_neg"]), q0
        assert np.array_equal(st[:, 2] > 1, want["valid_prec"]) and np.array_equal(st[:, 2], rel.sum(axis=1)), q0
        assert np.array_equal(topk.cpu().numpy()[:, :k], want["topk_idx"]), q0
        assert np.array_equal(st[:, 3], want["hits"]), q0
        assert not (want["topk_idx"] == (q0 + np.arange(nb))[:, None]).any()                      # a row never retrieves itself
