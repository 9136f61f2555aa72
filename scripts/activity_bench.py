#!/usr/bin/env python3
"""Device time of the band-limited activity gate (avex_amd.activity over csrc/activity.hip) on one hour of synthetic audio at 16 kHz,
against two yardsticks measured in the same call:

* the frames kernel (``avexhip_activity_frames``) against the ``avexhip_window_stats`` pass over the same resident waveform -- both read
  every sample once, so the ratio says what the transform costs over a plain reduction;
* the whole gate (``band_activity`` + ``select``, host planning included) against embedding the windows it removes with the BEATs
  encoder (synthetic weights, the shapes of the real model) -- what the gate saves.

    python scripts/activity_bench.py [--reps 5] [--hours 1.0] [--window-s 1.0] [--hop 256] [--no-encoder] [--out profiles/activity_bench.json]

The audio: -40 dBFS Gaussian noise with a 1.5 s, -10 dBFS tone at 3 kHz every 20 s.  Every leg is timed with device events after a
warm-up, the best of ``--reps``.  Nothing is gated: the script reports."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avex_amd import activity, recordings  # noqa: E402
from avex_amd._capi import check, lib  # noqa: E402

SR = 16000


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


def audio(hours):
    n = int(hours * 3600 * SR)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = 0.01 * torch.randn(n, device="cuda", generator=g)
    t = torch.arange(int(1.5 * SR), device="cuda", dtype=torch.float64) / SR
    tone = (10.0 ** -0.5 * torch.sin(2.0 * np.pi * 3000.0 * t)).to(torch.float32)
    for s in range(5 * SR, n - len(tone), 20 * SR):
        x[s:s + len(tone)] += tone
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--no-encoder", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    x = audio(a.hours)
    window_len = int(round(a.window_s * SR))
    ws = recordings.RecordingWindows([x], SR, window_len, window_len)
    gate = activity.ActivityGate([(2000, 8000)], snr_db=10.0, min_active_frames=2, hop=a.hop)
    act = activity.band_activity(ws, gate)
    stream = torch.cuda.current_stream().cuda_stream
    L, n, nb = lib(), ws.n_windows, len(act.bins)
    rec_host, rec_dev, tab = act._rec.ctypes.data, act._rec_dev.data_ptr(), activity._tables_on(x.device)
    legs = {
        "window_stats": lambda: check(L.avexhip_window_stats(ws.wav.data_ptr(), ws.wav.numel(), ws._table.ctypes.data, ws._table_dev.data_ptr(), n, window_len,
                                                             ws.energy.data_ptr(), ws.peak.data_ptr(), stream), "window_stats"),
        "frames": lambda: check(L.avexhip_activity_frames(ws.wav.data_ptr(), ws.wav.numel(), rec_host, rec_dev, 1, a.hop, act.bins.ctypes.data, nb, tab.data_ptr(),
                                                          act.total_frames, act.frame_energy.data_ptr(), stream), "activity_frames"),
        "floor": lambda: check(L.avexhip_activity_floor(act.frame_energy.data_ptr(), act.total_frames, rec_host, rec_dev, 1, a.hop, nb, act.floor.data_ptr(),
                                                        act.nonfinite_frames.data_ptr(), stream), "activity_floor"),
        "count": lambda: check(L.avexhip_activity_count(ws._table.ctypes.data, ws._table_dev.data_ptr(), act._win_rec.ctypes.data, act._win_rec_dev.data_ptr(), n,
                                                        rec_host, rec_dev, 1, a.hop, act.frame_energy.data_ptr(), act.total_frames, act.floor.data_ptr(), nb,
                                                        float(gate.floor_min), float(gate.ratio), act.n_frames.data_ptr(), act.active_frames.data_ptr(),
                                                        act.max_energy.data_ptr(), stream), "activity_count"),
        "select": lambda: act.select(),
        "whole_gate": lambda: activity.band_activity(ws, gate).select(),
    }
    out = {"hours": a.hours, "samples": int(x.numel()), "window_s": a.window_s, "hop": a.hop, "n_windows": n, "frames": act.total_frames, "bands": nb}
    for name, fn in legs.items():
        out[name + "_s"] = timed(fn, a.reps)
    host = act.select().cpu().numpy()
    kept = host[:int(host[n])].astype(np.int64)
    removed = np.setdiff1d(np.arange(n, dtype=np.int64), kept)
    out.update(kept=int(len(kept)), removed=int(len(removed)), frames_over_window_stats=out["frames_s"] / out["window_stats_s"],
               frames_read_GBps=4.0 * x.numel() / out["frames_s"] / 1e9, window_stats_read_GBps=4.0 * x.numel() / out["window_stats_s"] / 1e9)
    if not a.no_encoder and len(removed):
        import avex_amd
        from avex_amd import synth
        sd = synth.beats_state_dict(synth.BEATS_BASE_CFG, seed=0)
        model = avex_amd.build_model_from_spec(avex_amd.get_model_spec("esp_aves2_sl_beats_all").model_copy(deep=True), "cuda:0", return_features_only=True)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        model.eval()
        model.register_hooks_for_layers(["last_layer"])
        idx = torch.from_numpy(removed).to("cuda", torch.int32)

        def embed():
            with torch.no_grad():
                for lo in range(0, len(removed), 256):
                    wav, mask = ws.batch(idx[lo:lo + 256])
                    model.extract_embeddings({"raw_wav": wav, "padding_mask": mask}, aggregation="mean")

        out["embed_removed_s"] = timed(embed, max(1, min(a.reps, 2)))
        out["embed_windows_per_s"] = len(removed) / out["embed_removed_s"]
        out["embed_removed_over_whole_gate"] = out["embed_removed_s"] / out["whole_gate_s"]
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "the activity gate on synthetic audio (scripts/activity_bench.py)", "result": out}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
