#!/usr/bin/env python3
"""Device time of avex_amd.detection.decode_events at user-sized shapes, against two yardsticks measured in the same call on the same
scores: the device-to-host copy of the score matrix into pinned memory (the cheapest step of the host decode this replaces) and
``scores.clone()`` (one read and one write of the same bytes: the memory-bound picture).

    python scripts/events_bench.py [--reps 5] [--out profiles/events_bench.json]

Shapes: N = 2^20, C = 1;  N = 2^18, C = 64;  N = 2^16, C = 1024;  512 sequences of 2 048 windows, C = 32.  Scores are white noise averaged
over 8 windows and scaled to unit deviation, so events are a few windows long; thresholds on 1.5 / off 0.5.  Two rule sets: the plain one
(smooth 1, no merge, no minimum) and a typical one (5-window median, merge_gap 2, min_windows 3).  Every leg is timed with device events
after a warm-up, the best of ``--reps``; ``decode_events`` runs with ``max_events`` fixed to the count of a first call, so no leg
synchronises inside.

Acceptance: at every shape the decode takes less time than the device-to-host copy of its scores (exit status 1 otherwise).  The ratio to
``clone`` is reported, not gated."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import detection  # noqa: E402

SHAPES = [(1 << 20, 1, 1), (1 << 18, 64, 1), (1 << 16, 1024, 1), (512 * 2048, 32, 512)]
RULES = {"plain": dict(smooth=1, merge_gap=0, min_windows=1), "typical": dict(smooth=5, smooth_mode="median", merge_gap=2, min_windows=3)}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def scores_of(n, c, seed=0):
    """[n, c] fp32: the sum of 8 consecutive unit normals over sqrt(8), per class."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cs = torch.randn(n + 8, c, device="cuda", generator=g).cumsum(0)
    return ((cs[8:] - cs[:-8]) / 8.0 ** 0.5).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows, ok = [], True
    for n, c, r in SHAPES:
        x = scores_of(n, c)
        offsets = [n // r * j for j in range(r)] + [n]
        pinned = torch.empty((n, c), dtype=torch.float32).pin_memory()
        d2h = timed(lambda: pinned.copy_(x, non_blocking=True), a.reps)
        clone = timed(lambda: x.clone(), a.reps)
        for name, rule in RULES.items():
            kw = dict(seq_offsets=offsets, on=1.5, off=0.5, **rule)
            count = int(detection.decode_events(x, **kw)["count"])
            dec = timed(lambda: detection.decode_events(x, max_events=count, **kw), a.reps)
            row = {"n_windows": n, "n_classes": c, "n_sequences": r, "rule": name, "events": count, "score_bytes": 4 * n * c,
                   "decode_s": dec, "d2h_s": d2h, "clone_s": clone, "decode_over_d2h": dec / d2h, "decode_over_clone": dec / clone,
                   "read_GBps": 4 * n * c / dec / 1e9, "ok": dec < d2h}
            ok = ok and row["ok"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "decode_events against the device-to-host copy and the clone of its scores (scripts/events_bench.py)", "rows": rows}, f, indent=1)
    print("ACCEPTED" if ok else "NOT ACCEPTED: a decode took longer than the device-to-host copy of its scores", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
