#!/usr/bin/env python3
"""Device time of event scoring (avex_amd.annotations over csrc/annotations.hip) against what it replaces: the same events copied to
pinned host memory and walked by the NumPy reference (tests/_annotations_ref.py).

    python scripts/annotations_bench.py [--reps 5] [--log2 20] [--out profiles/annotations_bench.json]

* ``one_segment``: P = A = 2^log2 events of one class in one recording, a staggered chain (every event overlaps both neighbours of the
  other side by a fifth of their union) scored at IoU 0.15, so 2 P - 1 pairs go through the scan;
* ``many_segments``: 512 recordings x 32 classes, 16 predictions and 16 jittered reference events in each, at IoU 0.5.

``score_events_s`` and ``match_events_s`` are device-event times after a warm-up, the best of ``--reps``; ``host_copy_s`` is the copy of the
four columns to pinned memory with its synchronisation, ``host_walk_s`` the reference walk over them (once).  Nothing is gated: the
script reports, and checks that both sides found the same matches."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _annotations_ref as A  # noqa: E402
from avex_amd import annotations  # noqa: E402
from avex_amd.annotations import Annotations, WindowPlan  # noqa: E402

SR = 16000
CELL = 16


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


def one_segment(n):
    """Prediction i over cells 4 i .. 4 i + 2, reference event i two cells later: each shares one cell of five with both neighbours."""
    plan = WindowPlan([4 * (n + 1) * CELL], SR, CELL, CELL)
    i = np.arange(n, dtype=np.int64)
    rows = np.stack([np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), 4 * i, 4 * i + 2])
    lo = (4 * i + 2) * CELL
    ann = Annotations(np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), lo / SR, (lo + 3 * CELL) / SR, n_classes=1)
    return plan, ann, rows, 0.15


def many_segments(n_rec=512, n_classes=32, per=16):
    plan = WindowPlan([4 * per * CELL] * n_rec, SR, CELL, CELL)
    rng = np.random.default_rng(0)
    r, c, k = np.meshgrid(np.arange(n_rec), np.arange(n_classes), np.arange(per), indexing="ij")
    r, c, k = r.reshape(-1), c.reshape(-1), k.reshape(-1)
    first = 4 * per * r + 4 * k
    rows = np.stack([r, c, first, first + 2]).astype(np.int64)
    lo = 4 * k * CELL + rng.integers(0, CELL, len(k))
    hi = lo + 2 * CELL + rng.integers(0, CELL, len(k))
    ann = Annotations(r, c, lo / SR, hi / SR, n_classes=n_classes)
    return plan, ann, rows, 0.5


def run(name, plan, ann, rows, iou, reps):
    n = rows.shape[1]
    pred = {k: torch.from_numpy(rows[i].astype(np.int32)).cuda() for i, k in enumerate(("sequence", "class_id", "first", "last"))}
    pred["peak"] = torch.rand(n, device="cuda")
    ref = ann.reference_events(SR, len(plan.ranges))
    out = {"case": name, "n_pred": int(n), "n_ref": int(len(ref.lo)), "segments": int(len(ref.seg_offsets) - 1), "iou": iou}
    out["score_events_s"] = timed(lambda: annotations.score_events(pred, ann, plan, iou=iou), reps)
    out["match_events_s"] = timed(lambda: annotations.match_events(pred, ann, plan, iou=iou), reps)
    got = annotations.score_events(pred, ann, plan, iou=iou)
    pinned = {k: torch.empty(n, dtype=torch.int32).pin_memory() for k in ("sequence", "class_id", "first", "last")}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k, t in pinned.items():
        t.copy_(pred[k], non_blocking=True)
    torch.cuda.synchronize()
    out["host_copy_s"] = time.perf_counter() - t0
    cols = [pinned[k].numpy() for k in ("sequence", "class_id", "first", "last")]
    lo, hi = annotations.window_cells(plan)
    table = {k: getattr(ref, k) for k in ("lo", "hi", "seg_offsets", "n_ref")}
    t0 = time.perf_counter()
    want_p, want_r, _ = A.match(list(zip(*(c.tolist() for c in cols))), lo, hi, table, ann.n_classes, iou)
    out["host_walk_s"] = time.perf_counter() - t0
    out["matched"] = int((want_p >= 0).sum())
    out["same_matches"] = bool(np.array_equal(got["match_of_pred"].cpu().numpy(), want_p) and np.array_equal(got["match_of_ref"].cpu().numpy(), want_r))
    out["order_errors"] = int(got["order_errors"])
    out["host_over_device"] = (out["host_copy_s"] + out["host_walk_s"]) / out["score_events_s"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    results = [run("one_segment", *one_segment(1 << a.log2), a.reps), run("many_segments", *many_segments(), a.reps)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "event scoring against annotations, device against a host walk (scripts/annotations_bench.py)", "results": results}, f, indent=1)
    return 0 if all(r["same_matches"] and r["order_errors"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
