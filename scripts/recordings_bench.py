#!/usr/bin/env python3
"""A recording -> one embedding per window: what the window kernels cost beside the encoder and beside the per-window ingest.

    python scripts/recordings_bench.py [--minutes 10] [--reps 3] [--out profiles/recordings_bench.json]

Workload: one synthetic recording (16-bit mono WAV at 16 kHz held in memory, 30 s of noise alternating with 30 s of exact silence),
10 s windows, hops of 10 s and of 1 s, without a gate and with one (min_rms_db = -40: the silent windows go).  Per hop and gate, in one
process, after a warm-up, best of --reps with the spread, wall clock around a device synchronise:
  (a) stats + select + gather: from the resident waveform to every kept window's row and mask (avexhip_window_stats once, then
      avexhip_window_select with a gate and the copy of its list, avexhip_window_gather in batches of 256);
  (b) the encoder alone on rows that are already there (synthetic BEATs-base, extract_embeddings with aggregation="mean", batches of 256);
  (c) the same rows from the parent commit's API: ingest.load_batch([file] * k, starts=...) in chunks of --chunk windows, which stages
      the file's payload once per window (a gate cannot be applied before the rows exist, so (c) always builds every window);
  (d) the same rows from load_audio and torch ops (slice, F.pad, stack, arange >= valid), the other route a user has today.
load_s is the one decode of the file that (a) and (d) start from.  (a) / (b) and (a) / (c) are recorded per case; rows of (a), (c) and
(d) are compared with torch.equal in the warm-up."""
import argparse
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
import avex_amd  # noqa: E402
from avex_amd import ingest, recordings, synth  # noqa: E402

SR, WINDOW_S, GATE_DB, BATCH = 16000, 10.0, -40.0, 256


def make_recording(minutes, seed=0):
    rng = np.random.default_rng(seed)
    pcm = (rng.standard_normal(int(minutes * 60 * SR)) * 3000).astype(np.int16)
    for s in range(0, len(pcm), 60 * SR):
        pcm[s + 30 * SR:s + 60 * SR] = 0
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(SR)
        w.writeframes(pcm.tobytes())
    return buf.getvalue()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def windows_path(wave_dev, hop_len, gate, keep_rows=False):
    """(a): the resident waveform -> rows and masks of the kept windows, in batches."""
    ws = recordings.RecordingWindows([wave_dev], SR, int(WINDOW_S * SR), hop_len)
    rows = []
    if gate:
        sel = ws.select(GATE_DB)
        n = int(sel[-1].item())                       # the one host synchronisation of a gated call
        for lo in range(0, n, BATCH):
            out = ws.batch(sel[lo:min(lo + BATCH, n)])
            if keep_rows:
                rows.append(out)
        return ws, sel[:n].cpu().numpy() if keep_rows else n, rows
    for lo in range(0, ws.n_windows, BATCH):
        out = ws.batch(lo, min(lo + BATCH, ws.n_windows))
        if keep_rows:
            rows.append(out)
    return ws, np.arange(ws.n_windows) if keep_rows else ws.n_windows, rows


def load_batch_path(data, starts, chunk, keep_rows=False):
    """(c): every window through the parent commit's per-file ingest."""
    rows = []
    T = int(WINDOW_S * SR)
    for lo in range(0, len(starts), chunk):
        part = starts[lo:lo + chunk]
        wav, mask, _ = ingest.load_batch([data] * len(part), SR, T, starts=part)
        if keep_rows:
            rows.append((wav, mask))
    return rows


def torch_path(wave_dev, starts, valids, keep_rows=False):
    """(d): slices of the resident waveform with torch ops."""
    rows = []
    T = int(WINDOW_S * SR)
    ar = torch.arange(T, device=wave_dev.device)
    for lo in range(0, len(starts), BATCH):
        wav = torch.stack([F.pad(wave_dev[s:s + v], (0, T - v)) for s, v in zip(starts[lo:lo + BATCH], valids[lo:lo + BATCH])])
        mask = ar[None, :] >= torch.tensor(valids[lo:lo + BATCH], device=wave_dev.device)[:, None]
        if keep_rows:
            rows.append((wav, mask))
    return rows


def encoder_path(model, ws, index):
    """(b): the encoder on the kept windows' rows; the rows are gathered outside the timed region, batch by batch."""
    total = 0.0
    idx = torch.as_tensor(index, dtype=torch.int32, device=ws.wav.device)
    for lo in range(0, len(index), BATCH):
        wav, mask = ws.batch(idx[lo:lo + BATCH])
        dt, _ = wall(lambda: model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation="mean"))
        total += dt
    return total


def best(fn, reps):
    t = [fn() for _ in range(reps)]
    return {"best_s": min(t), "all_s": t, "spread_s": max(t) - min(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16, help="windows per load_batch call in (c): each stages the whole file once")
    ap.add_argument("--layers", type=int, default=12, help="encoder layers of the synthetic BEATs model")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "recordings_bench.json"))
    args = ap.parse_args()
    data = make_recording(args.minutes)
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=args.layers)
    model = avex_amd.beats_model.Model(device="cuda", init_config=cfg, return_features_only=True).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.beats_state_dict(cfg, seed=0).items()}, strict=False)
    model.register_hooks_for_layers(["last_layer"])
    wall(lambda: ingest.load_audio(data, SR))
    load = best(lambda: wall(lambda: ingest.load_audio(data, SR))[0], args.reps)
    wave_dev = ingest.load_audio(data, SR)[0]
    res = {"device": torch.cuda.get_device_name(0), "minutes": args.minutes, "samples": int(wave_dev.numel()), "file_bytes": len(data),
           "window_s": WINDOW_S, "gate_min_rms_db": GATE_DB, "batch": BATCH, "load_batch_chunk": args.chunk, "encoder": f"synthetic BEATs-base, {args.layers} layers, f16",
           "load_s": load, "cases": []}
    for hop_s in (10.0, 1.0):
        hop_len = int(hop_s * SR)
        # warm-up of every path at this shape, and the check that they build the same rows
        ws, index, rows_a = windows_path(wave_dev, hop_len, False, keep_rows=True)
        starts, valids = ws.starts.tolist(), ws.valids.tolist()
        rows_c, rows_d = load_batch_path(data, starts[:2 * args.chunk], args.chunk, True), torch_path(wave_dev, starts, valids, True)
        wav_a, mask_a = torch.cat([w for w, _ in rows_a]), torch.cat([m for _, m in rows_a])
        same_d = bool(torch.equal(wav_a, torch.cat([w for w, _ in rows_d])) and torch.equal(mask_a, torch.cat([m for _, m in rows_d])))
        nc = sum(w.shape[0] for w, _ in rows_c)
        same_c = bool(torch.equal(wav_a[:nc], torch.cat([w for w, _ in rows_c])) and torch.equal(mask_a[:nc], torch.cat([m for _, m in rows_c])))
        del rows_a, rows_c, rows_d, wav_a, mask_a
        encoder_path(model, ws, index[:BATCH])
        c = best(lambda: wall(lambda: load_batch_path(data, starts, args.chunk))[0], 1 if len(starts) > 100 else args.reps)
        d = best(lambda: wall(lambda: torch_path(wave_dev, starts, valids))[0], args.reps)
        for gate in (False, True):
            _, kept, _ = windows_path(wave_dev, hop_len, gate, keep_rows=True)
            a = best(lambda: wall(lambda: windows_path(wave_dev, hop_len, gate))[0], args.reps)
            b = best(lambda: encoder_path(model, ws, kept), args.reps)
            n, k = ws.n_windows, len(kept)
            res["cases"].append({"hop_s": hop_s, "gate": gate, "windows": n, "kept": k, "rows_equal_load_batch": same_c, "rows_equal_torch": same_d,
                                 "a_windows": dict(a, us_per_window=1e6 * a["best_s"] / n), "b_encoder": dict(b, us_per_window=1e6 * b["best_s"] / max(k, 1)),
                                 "c_load_batch": dict(c, us_per_window=1e6 * c["best_s"] / n), "d_torch_slices": dict(d, us_per_window=1e6 * d["best_s"] / n),
                                 "a_over_b": a["best_s"] / b["best_s"], "a_over_c": a["best_s"] / c["best_s"], "a_over_d": a["best_s"] / d["best_s"],
                                 "a_plus_b_over_ungated_b": None})
    for case in res["cases"]:          # what the gate saves end to end: (a) + (b) of the case over (b) of the same hop without a gate
        full = next(c for c in res["cases"] if c["hop_s"] == case["hop_s"] and not c["gate"])
        case["a_plus_b_over_ungated_b"] = (case["a_windows"]["best_s"] + case["b_encoder"]["best_s"]) / full["b_encoder"]["best_s"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
