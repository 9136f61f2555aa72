#!/usr/bin/env python3
"""Device time of the sound-event regions (avex_amd.regions over csrc/regions.hip) on 8 recordings of 10 minutes of synthetic audio at
16 kHz, hop 128, snr_db 10, against the statistics kernel of the acoustic indices (``avexhip_soundscape_frames``) over the same resident
waveform in the same run -- the same frames through the same transform -- and against a CPU chain (``torch.fft.rfft`` of the frames of
ONE of the recordings, then ``scipy.ndimage.label`` on the device's mask of that recording).

    python scripts/regions_bench.py [--reps 5] [--recordings 8] [--minutes 10] [--hop 128] [--snr-db 10] [--out profiles/regions_bench.json]

The audio is that of scripts/activity_bench.py, cut into the recordings.  Every entry point is timed with device events after one
warm-up call, the best of ``--reps``: ``cells`` is one launch, ``count`` three (the prefix of the frames' set cells), ``label`` nine (init,
union, flatten, the roots' prefix, boxes, the kept regions' prefix), ``rows`` one; ``whole_call`` is ``find_regions`` end to end with its
two host reads.  The split of ``label`` by kernel comes from ``rocprofv3 --kernel-trace --stats -- python scripts/regions_bench.py``.
``label_bytes`` is what the labelling kernels must move at the least, ``label_gbps`` that over the time of
count + label + rows.  Nothing is gated: the script reports."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from activity_bench import SR, audio, timed  # noqa: E402
from avex_amd import activity, measurements, recordings, regions, soundscape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--hop", type=int, default=128)
    ap.add_argument("--snr-db", type=float, default=10.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = int(a.minutes * 60 * SR)
    x = audio(a.recordings * a.minutes / 60.0)
    ws = recordings.RecordingWindows([x[r * n:(r + 1) * n] for r in range(a.recordings)], SR, SR, SR)
    stream = torch.cuda.current_stream().cuda_stream
    st = soundscape.spectral_stats(ws, soundscape.IndexSpec(hop=a.hop, segment_s=60.0))
    tab = activity._tables_on(x.device)
    noise = measurements.noise_spectrum(st)
    spec = regions.RegionSpec(hop=a.hop, snr_db=a.snr_db)
    out = {"recordings": a.recordings, "minutes": a.minutes, "samples": int(x.numel()), "hop": a.hop, "snr_db": a.snr_db, "frames": st.total_frames,
           "soundscape_stats_s": timed(lambda: st._frames(stream, tab), a.reps)}

    best = {}

    def hook(name, launch):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        launch()
        e.record()
        torch.cuda.synchronize()
        best[name] = min(best.get(name, float("inf")), b.elapsed_time(e) * 1e-3)

    r = regions.find_regions(ws, spec, noise_power=noise)      # warm-up
    for _ in range(a.reps):
        r = regions.find_regions(ws, spec, noise_power=noise, _timed=hook)
    F, cells, rt = st.total_frames, r.n_cells, spec.reach[0]
    out.update({f"{k}_s": v for k, v in best.items()})
    out["total_s"] = sum(best.values())
    out["whole_call_s"] = timed(lambda: regions.find_regions(ws, spec, noise_power=noise), a.reps)
    out["cells_over_soundscape_stats"] = best["cells"] / out["soundscape_stats_s"]
    out.update(set_cells=cells, cell_fraction=cells / (F * 257.0), regions_found=int(r.n_found), regions_kept=int(r["recording"].shape[0]))
    # the least the labelling moves: the 36 bytes of a frame's words read by the two passes of the count, the union (the frame and its
    # rt successors) and the boxes, the frame's offset written once and read beside the words; per set cell 5 words initialised, the
    # parent read and hooked by the union, read and written by the flatten, read by the two passes of the roots' prefix and by the
    # boxes, the rank written and read, one atomic
    out["label_bytes"] = F * (36 * (4 + rt) + 4 * (3 + rt)) + cells * 4 * (5 + 2 + 2 + 2 + 1 + 2 + 1)
    out["label_gbps"] = out["label_bytes"] / (best["count"] + best["label"] + best["rows"]) / 1e9

    if not a.no_cpu:                                             # the CPU chain, over recording 0
        F0 = activity.frame_count(n, a.hop)
        host = x[:n].cpu()
        window = torch.from_numpy(activity.tables()[:512].copy())
        t0 = time.perf_counter()
        P = torch.fft.rfft(host.unfold(0, 512, a.hop) * window).abs().square_()
        mask_cpu = P > torch.maximum(noise[0].cpu() * float(spec.ratio), torch.zeros(()))
        out["cpu_rfft_s"] = time.perf_counter() - t0
        out["cpu_frames"] = F0
        try:
            from scipy import ndimage
            mask = r.cells[:F0].cpu().numpy().view(np.uint32)
            bits = ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(F0, -1)[:, :257].astype(bool)
            t0 = time.perf_counter()
            _, found = ndimage.label(bits, structure=np.ones((3, 3)))
            out["cpu_label_s"] = time.perf_counter() - t0
            out["cpu_regions"] = int(found)
            out["cpu_mask_differs"] = int((bits != mask_cpu.numpy()).sum())
        except ImportError:
            pass
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "sound-event regions on synthetic audio (scripts/regions_bench.py)", "result": out}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
