#!/usr/bin/env python3
"""Files -> model batch: the per-file path against avex_amd.ingest.load_batch.

    python scripts/ingest_batch_bench.py [--clips 256] [--out profiles/ingest_batch.json]
    python scripts/ingest_batch_bench.py --only a|b --reps 1          (one path alone, for a kernel trace of its launches)
    python scripts/ingest_batch_bench.py --launch-counts A.csv B.csv  (adds the rows of two kernel-trace CSVs to the JSON)

Workload: --clips synthetic WAV files held in memory (16-bit, 44.1 kHz, stereo, 10 .. 60 s), target 16 kHz, 10 s windows from the start.
  (a) the per-file path: load_audio per file, then torch slice / pad / stack and the mask;
  (b) load_batch.
Both start from the files' bytes and end with wav [B, T] and mask [B, T] on the device (wall clock around a device synchronise: host
parsing and staging are part of the cost).  One warm-up, then --reps repeats of each path, alternating, in one process; the best and
the spread are recorded, and clips/s beside the BEATs encoder's 10 k clips/s."""
import argparse
import csv
import io
import json
import os
import sys
import time
import wave

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import ingest  # noqa: E402

SR, TARGET_SR, SECONDS = 44100, 16000, 10
ENCODER_CLIPS_PER_S = 10000.0


def make_files(n, seed=0):
    rng = np.random.default_rng(seed)
    files = []
    for secs in rng.uniform(10.0, 60.0, n):
        pcm = rng.integers(-20000, 20000, (int(secs * SR), 2), dtype=np.int16)
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(SR)
            w.writeframes(pcm.tobytes())
        files.append(buf.getvalue())
    return files


def per_file(files, T):
    rows, masks = [], []
    for f in files:
        x, _ = ingest.load_audio(f, TARGET_SR)
        x = x[:T]
        rows.append(F.pad(x, (0, T - x.numel())))
        masks.append(torch.arange(T, device=x.device) >= x.numel())
    return torch.stack(rows), torch.stack(masks)


def batched(files, T):
    wav, mask, _ = ingest.load_batch(files, TARGET_SR, T)
    return wav, mask


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("a", "b"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ingest_batch.json"))
    ap.add_argument("--launch-counts", nargs=2, metavar=("A_CSV", "B_CSV"))
    args = ap.parse_args()
    if args.launch_counts:
        res = json.load(open(args.out))
        for key, path in zip(("a_per_file", "b_load_batch"), args.launch_counts):
            with open(path) as f:
                res[key]["kernel_launches"] = sum(1 for _ in csv.DictReader(f))
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps({k: res[k]["kernel_launches"] for k in ("a_per_file", "b_load_batch")}))
        return
    files = make_files(args.clips)
    T = SECONDS * TARGET_SR
    paths = {"a": ("a_per_file", per_file), "b": ("b_load_batch", batched)}
    if args.only:
        for _ in range(args.reps):
            wall(lambda: paths[args.only][1](files, T))
        return
    (_, (wa, ma)), (_, (wb, mb)) = wall(lambda: per_file(files, T)), wall(lambda: batched(files, T))      # the warm-up, and a check
    res = {"clips": args.clips, "file_bytes": sum(len(f) for f in files), "target_samples": T, "device": torch.cuda.get_device_name(0),
           "rows_bit_identical": bool(torch.equal(wa, wb) and torch.equal(ma, mb)), "encoder_clips_per_s": ENCODER_CLIPS_PER_S}
    del wa, ma, wb, mb
    times = {"a": [], "b": []}
    for _ in range(args.reps):
        for k in ("a", "b"):
            times[k].append(wall(lambda: paths[k][1](files, T))[0])
    for k, (name, _) in paths.items():
        t = times[k]
        res[name] = {"best_s": min(t), "all_s": t, "spread_s": max(t) - min(t), "clips_per_s": args.clips / min(t),
                     "share_of_encoder_rate": args.clips / min(t) / ENCODER_CLIPS_PER_S}
    res["speedup_b_over_a"] = res["a_per_file"]["best_s"] / res["b_load_batch"]["best_s"]
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
