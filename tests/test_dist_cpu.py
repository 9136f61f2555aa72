"""N > 1 data-parallel path on CPU: world_size-2 gloo processes shard a batch, embed their slice and
all-gather pooled embeddings; the result must equal the single-process result row for row."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from avex_amd import dist as adist


def test_shard_bounds_cover_everything():
    for n in (0, 1, 7, 8, 9, 256, 2048, 2051):
        for w in (1, 2, 3, 8):
            spans = [adist.shard_bounds(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    assert adist.shard_bounds(2048, 3, 8) == (768, 1024)        # BASELINE config C4: 256 clips per GPU


def _embed(wav: torch.Tensor) -> torch.Tensor:
    """Stand-in for model.extract_embeddings(...): any per-clip function works, clips are independent."""
    feats = torch.stack([wav.mean(1), wav.std(1), wav.abs().max(1)[0], (wav ** 2).mean(1)], dim=1)
    return feats.float()


def _worker(rank, world, port, n_clips, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    r, w, _ = adist.init_distributed(backend="gloo")
    assert (r, w) == (rank, world)
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(n_clips, 4000, generator=g)
    full = adist.extract_embeddings_sharded(_embed, wav)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), full.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_clips", [8, 7, 1])
def test_two_rank_gloo_all_gather(tmp_path, n_clips):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, n_clips, str(tmp_path)), nprocs=2, join=True)
    g = torch.Generator().manual_seed(0)
    ref = _embed(torch.randn(n_clips, 4000, generator=g)).numpy()
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npy")
        assert got.shape == ref.shape and np.array_equal(got, ref)       # every rank holds every row, in clip order


def _reinit_worker(rank, world, port, out_dir):
    """init_distributed -> gather -> torch.distributed destroyed and re-initialised OUTSIDE init_distributed -> gather again: the second
    gather must not run on the first world's group (_WORK_GROUP was never cleared); then shutdown() and a clean third start."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    adist.init_distributed(backend="gloo")
    g1 = adist.work_group()
    assert g1 is not None
    wav = torch.randn(6, 1000, generator=torch.Generator().manual_seed(1))
    a = adist.extract_embeddings_sharded(_embed, wav)
    dist.barrier()
    dist.destroy_process_group()                      # the caller tears the world down itself ...
    assert adist.work_group() is None                 # ... and the stale group is dropped, not handed out
    os.environ["MASTER_PORT"] = str(port + 1)
    dist.init_process_group(backend="gloo")           # ... and brings up a new one without init_distributed
    b = adist.extract_embeddings_sharded(_embed, wav)  # default group of the new world
    adist.init_distributed(backend="gloo")            # gives the data path its own group in the new world
    g2 = adist.work_group()
    assert g2 is not None and g2 is not g1
    c = adist.extract_embeddings_sharded(_embed, wav)
    dist.barrier()
    adist.shutdown()
    assert not dist.is_initialized() and adist.work_group() is None
    os.environ["MASTER_PORT"] = str(port + 2)
    adist.init_distributed(backend="gloo")
    d = adist.extract_embeddings_sharded(_embed, wav)
    dist.barrier()
    adist.shutdown()
    ref = _embed(wav)
    assert all(torch.equal(x, ref) for x in (a, b, c, d))
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")


def test_work_group_does_not_outlive_its_world(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_reinit_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()


def test_single_process_is_a_no_op():
    wav = torch.randn(3, 100)
    assert torch.equal(adist.extract_embeddings_sharded(_embed, wav), _embed(wav))


def test_bench_multi_rank_control_flow(tmp_path):
    """bench.py launched exactly as the driver launches it for N > 1 (torch.distributed.run, one rank per device), on the CPU
    with gloo and a stub encoder (--cpu-dry-run): rendezvous, rank-0-builds barrier, warm-up, barrier-bracketed timing, MAX over
    ranks, the per-step all-gather of pooled rows and the single JSON line from rank 0."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4",
           "--cpu-dry-run"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                   # ONE line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["unit"] == "clips/s"
    assert d["config"]["global_batch"] == 8 and d["config"]["parallelism"] == "dp2" and d["value"] > 0
    assert "RCCL all-gather" in d["config"]["workload"]


def test_bench_launches_its_own_ranks_from_a_plain_shell(tmp_path):
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment (how the driver starts the 1-GPU run, with N > 1): the parent starts
    torch.distributed.run as a child before anything touches a GPU, relays rank 0's single JSON line and the exit code.  The dry run also
    checks the gathered matrix against the clip-index-keyed generator (row r*B + i = clip r*B + i)."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "3",
                        "--cpu-dry-run", "--full"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["backend"] == "gloo"
    assert d["config"]["gathered_rows_in_clip_order"] is True and d["config"]["global_batch"] == 6


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path, gpus):
    """A plain run (no --full) times exactly --steps steps, prints only the headline line, and --dump-outputs writes what the timed path
    returned at its last step: the stub's closed form of every clip of the job, in clip order (all ranks' rows, gathered)."""
    import json, subprocess, sys
    from avex_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus), "--steps", "3", "--warmup", "1", "--batch", "3",
                        "--cpu-dry-run", "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and "checklist" not in d["config"] and d["config"]["gathered_rows_in_clip_order"] is None
    assert not {"parity", "power", "configs", "cpu_baseline"} & set(d)
    assert sorted(os.listdir(tmp_path / "dump")) == ["pooled.npy"]
    got = np.load(tmp_path / "dump" / "pooled.npy")
    want = synth.noise_clips(gpus * 3, 160000, seed=0)[:, :768] * 2.0
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_bench_dump_over_budget_is_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    """--dump-outputs above its byte budget keeps whole rows, in row order, chosen by a fixed seed: two dumps of the same output agree."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 768 * 4)
    out = torch.arange(40 * 768, dtype=torch.float32).reshape(40, 768)
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "pooled.npy"), np.load(tmp_path / "b" / "pooled.npy")
    assert a.shape == (10, 768) and a.dtype == np.float32 and np.array_equal(a, b)
    rows = a[:, 0].astype(np.int64) // 768
    assert np.array_equal(a, out.numpy()[rows]) and (np.diff(rows) > 0).all()


def test_bench_refuses_mismatched_world(tmp_path):
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--cpu-dry-run"], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


# ------------------------------------------------------------------ pipelined (non-blocking) gather and the sharded harness loop
class _StubModel:
    """Enough of the model contract for the extraction loop: hooks bookkeeping + a per-clip extract_embeddings."""
    disable_layerdrop = False

    def __init__(self, list_output: bool) -> None:
        self.list_output = list_output
        self.calls = []

    def register_hooks_for_layers(self, layers):
        return ["layer.a", "layer.b"] if self.list_output else ["layer.a"]

    def deregister_all_hooks(self):
        pass

    def extract_embeddings(self, x, aggregation="mean"):
        wav = x["raw_wav"] if isinstance(x, dict) else x
        self.calls.append(int(wav.shape[0]))
        e = _embed(wav)
        if self.list_output:
            return [e.unsqueeze(1).repeat(1, 3, 1), (2.0 * e).unsqueeze(1).repeat(1, 3, 1)]       # (B, T', D) per layer, aggregation "none"
        return e


def _batches(n_batches, sizes):
    g = torch.Generator().manual_seed(1)
    out = []
    for i in range(n_batches):
        b = sizes[i % len(sizes)]
        out.append({"raw_wav": torch.randn(b, 2000, generator=g), "padding_mask": torch.zeros(b, 2000, dtype=torch.bool),
                    "label": torch.arange(b) + 100 * i})
    return out


def _pipe_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    adist.init_distributed(backend="gloo")
    from avex_amd.extraction import extract_embeddings_in_memory
    # (a) PipelinedGather against the blocking gather, equal and ragged splits, results one step late
    g = torch.Generator().manual_seed(5)
    pg = adist.PipelinedGather()
    got, want = [], []
    for n_total in (8, 7, 8, 3, 1, 6):
        full = torch.randn(n_total, 5, generator=g)
        lo, hi = adist.shard_bounds(n_total, rank, world)
        want.append(full)
        prev = pg.push(full[lo:hi].clone(), n_total)
        if prev is not None:
            got.append(prev.clone())
    got.append(pg.flush().clone())
    assert pg.flush() is None
    ok_a = len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    # (b) the harness loop, sharded: every rank iterates the same batches and returns the single-device result
    res = {}
    for list_output in (False, True):
        model = _StubModel(list_output)
        emb, labels, dims = extract_embeddings_in_memory(model, _batches(5, (6, 5, 1)), ["last_layer"], "cpu",
                                                         aggregation="none" if list_output else "mean", sharded=True)
        res[list_output] = ({k: v.numpy() for k, v in emb.items()}, labels.numpy(), dims, model.calls)
    # (c) sharding is opt-in: by default every rank embeds its own whole batches (what a DistributedSampler set-up needs) ...
    model = _StubModel(False)
    own = _batches(3, (4,))
    for b in own:
        b["raw_wav"] = b["raw_wav"] + rank      # a different batch per rank
    emb, labels, dims = extract_embeddings_in_memory(model, own, ["last_layer"], "cpu")
    ok_c = model.calls == [4, 4, 4] and torch.equal(next(iter(emb.values())), torch.cat([_embed(b["raw_wav"]) for b in own]))
    # ... and asking for it with different batches per rank is refused instead of gathering unrelated rows
    try:
        extract_embeddings_in_memory(_StubModel(False), own, ["last_layer"], "cpu", sharded=True)
        ok_c = False
    except RuntimeError as e:
        ok_c = ok_c and "same batches" in str(e)
    np.save(os.path.join(out_dir, f"optin_ok_r{rank}.npy"), np.array([int(ok_c)]))
    np.save(os.path.join(out_dir, f"pipe_ok_r{rank}.npy"), np.array([int(ok_a)]))
    import pickle
    with open(os.path.join(out_dir, f"loop_r{rank}.pkl"), "wb") as f:
        pickle.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


def test_pipelined_gather_and_sharded_extraction_loop(tmp_path):
    import pickle
    from avex_amd.extraction import extract_embeddings_in_memory
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_pipe_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    ref = {}
    for list_output in (False, True):          # the single-process loop is the reference
        emb, labels, dims = extract_embeddings_in_memory(_StubModel(list_output), _batches(5, (6, 5, 1)), ["last_layer"], "cpu",
                                                         aggregation="none" if list_output else "mean")
        ref[list_output] = ({k: v.numpy() for k, v in emb.items()}, labels.numpy(), dims)
    for r in range(2):
        assert np.load(tmp_path / f"pipe_ok_r{r}.npy")[0] == 1
        assert np.load(tmp_path / f"optin_ok_r{r}.npy")[0] == 1      # default = unsharded; sharded=True with different batches per rank is refused
        with open(tmp_path / f"loop_r{r}.pkl", "rb") as f:
            res = pickle.load(f)
        for list_output in (False, True):
            emb, labels, dims, calls = res[list_output]
            remb, rlabels, rdims = ref[list_output]
            assert sorted(emb) == sorted(remb) and dims == rdims and np.array_equal(labels, rlabels)
            for k in remb:
                assert np.array_equal(emb[k], remb[k]), (r, list_output, k)              # every rank: every row, in clip order
            # each rank embedded only its share of every batch (a one-clip batch still costs the idle rank one probe clip)
            assert calls == ([3, 3, 1, 3, 3] if r == 0 else [3, 2, 1, 3, 2]), calls


def test_bench_control_flow_at_eight_ranks(tmp_path):
    """BASELINE config C4's process layout (8 ranks) on the CPU with gloo and the stub encoder: rendezvous, pipelined gather, the
    clip-order check over all 8 shards, one JSON line."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1", "--batch", "2", "--cpu-dry-run", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp8" and d["config"]["world_size"] == 8
    assert d["config"]["gathered_rows_in_clip_order"] is True
    assert d["config"]["all_gather"]["blocking_ms"] > 0 and d["config"]["all_gather"]["bytes_per_rank"] == 2 * 768 * 4
    # what a first real 8-GPU run needs in order to say WHERE it is slow: every rank's own step time, the slowest rank, and the time
    # the compute stream waited for gathers that had not finished under the next step
    pr = d["config"]["per_rank"]
    assert len(pr["ms_per_step"]) == 8 and pr["ms_per_step_min"] <= pr["ms_per_step_max"] and 0 <= pr["slowest_rank"] < 8
    assert pr["ms_per_step_max"] <= d["ms_per_step"] * 1.001 + 1e-6          # the line's time is the max over ranks (plus the closing barrier)
    assert pr["exposed_gather_ms_per_step_max"] >= pr["exposed_gather_ms_per_step_mean"] >= 0
    assert d["config"]["all_gather"]["exposed_ms"] == pr["exposed_gather_ms_per_step_max"]
    # DESIGN.md section 5's five-line checklist, evaluated by the bench itself: in the JSON and as one line on stderr (the timing items -- exposed
    # gather, per-rank spread -- are reported, not asserted: eight CPU processes on a shared host are not eight boards)
    ck = d["config"]["checklist"]
    assert len(ck) == 5 and ck["world_size == n_gpus"] is True and ck["gathered rows in clip order"] is True
    assert any(k.startswith("backend") for k in ck) and all(isinstance(v, bool) for v in ck.values())
    verdict = [ln for ln in r.stderr.splitlines() if ln.startswith("[bench] multi-GPU checklist (8 ranks):")]
    assert len(verdict) == 1 and ("all 5 hold" in verdict[0] or "FAILED:" in verdict[0])


def test_bench_rendezvous_failure_is_loud_and_names_the_rank(tmp_path):
    """A rank whose peers never arrive must not hang the job: init_process_group has a timeout (AVEX_AMD_DIST_TIMEOUT_S), the rank says
    which rank it is and what it was waiting for, and exits with code 3."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="1", LOCAL_RANK="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29431", AVEX_AMD_DIST_TIMEOUT_S="5")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "2", "--cpu-dry-run"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "rank 1/2" in r.stderr and "FAILED" in r.stderr and "MASTER_PORT=29431" in r.stderr
