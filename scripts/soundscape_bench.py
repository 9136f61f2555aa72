#!/usr/bin/env python3
"""Device time of the acoustic indices (avex_amd.soundscape over csrc/soundscape.hip) on one hour of synthetic audio at 16 kHz, hop 256,
60 s segments, against two yardsticks measured in the same run over the same resident waveform:

* ``avexhip_window_stats`` -- a plain reduction that reads every sample once;
* ``avexhip_activity_frames`` (one band) -- the same frames through the pair-packed transform, collapsed to a band sum.

    python scripts/soundscape_bench.py [--reps 5] [--hours 1.0] [--hop 256] [--segment-s 60] [--out profiles/soundscape_bench.json]

The audio is that of scripts/activity_bench.py: -40 dBFS Gaussian noise with a 1.5 s, -10 dBFS tone at 3 kHz every 20 s.  Every leg is timed
with device events after one warm-up, the best of ``--reps``.  Nothing is gated: the script reports."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from activity_bench import SR, audio, timed  # noqa: E402
from avex_amd import activity, recordings, soundscape  # noqa: E402
from avex_amd._capi import check, lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--segment-s", type=float, default=60.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    x = audio(a.hours)
    ws = recordings.RecordingWindows([x], SR, SR, SR)
    spec = soundscape.IndexSpec(hop=a.hop, segment_s=a.segment_s)
    ind = soundscape.acoustic_indices(ws, spec)
    st = ind.stats
    act = activity.band_activity(ws, activity.ActivityGate([(2000, 8000)], hop=a.hop))
    stream = torch.cuda.current_stream().cuda_stream
    L, n, tab = lib(), ws.n_windows, activity._tables_on(x.device)
    legs = {
        "window_stats": lambda: check(L.avexhip_window_stats(ws.wav.data_ptr(), ws.wav.numel(), ws._table.ctypes.data, ws._table_dev.data_ptr(), n, SR,
                                                             ws.energy.data_ptr(), ws.peak.data_ptr(), stream), "window_stats"),
        "activity_frames": lambda: check(L.avexhip_activity_frames(ws.wav.data_ptr(), ws.wav.numel(), act._rec.ctypes.data, act._rec_dev.data_ptr(), 1, a.hop,
                                                                   act.bins.ctypes.data, len(act.bins), tab.data_ptr(), act.total_frames,
                                                                   act.frame_energy.data_ptr(), stream), "activity_frames"),
        "stats": lambda: st._frames(stream, tab),
        "reduce": lambda: st._reduce(stream),
        "indices": lambda: ind._launch(stream),
        "whole_call": lambda: soundscape.acoustic_indices(ws, spec),
    }
    out = {"hours": a.hours, "samples": int(x.numel()), "hop": a.hop, "segment_s": a.segment_s, "segment_frames": st.segment_frames, "frames": st.total_frames,
           "segments": st.n_segments, "runs": st.n_runs, "partials_bytes": st._partials_bytes}
    for name, fn in legs.items():
        out[name + "_s"] = timed(fn, a.reps)
    out.update(stats_over_window_stats=out["stats_s"] / out["window_stats_s"], stats_over_activity_frames=out["stats_s"] / out["activity_frames_s"],
               stats_read_GBps=4.0 * x.numel() / out["stats_s"] / 1e9, window_stats_read_GBps=4.0 * x.numel() / out["window_stats_s"] / 1e9)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "acoustic indices on synthetic audio (scripts/soundscape_bench.py)", "result": out}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
