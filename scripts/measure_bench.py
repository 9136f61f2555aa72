#!/usr/bin/env python3
"""Device time of the event measurements (avex_amd.measurements over csrc/measure.hip) on one hour of synthetic audio at 16 kHz, hop 256:
3 600 one-second events that tile the hour, then 60 one-minute events, against the statistics kernel of the acoustic indices
(``avexhip_soundscape_frames``, 60 s segments) over the same resident waveform in the same run -- the same frames through the same
transform.

    python scripts/measure_bench.py [--reps 5] [--hours 1.0] [--hop 256] [--out profiles/measure_bench.json]

The audio is that of scripts/activity_bench.py.  Every leg is timed with device events after one warm-up, the best of ``--reps``;
``whole_call`` is ``measure_boxes`` end to end (host plan, table upload, allocations, two launches, the derived columns).  Nothing is gated:
the script reports."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from activity_bench import SR, audio, timed  # noqa: E402
from avex_amd import activity, measurements, recordings, soundscape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    x = audio(a.hours)
    ws = recordings.RecordingWindows([x], SR, SR, SR)
    stream = torch.cuda.current_stream().cuda_stream
    st = soundscape.spectral_stats(ws, soundscape.IndexSpec(hop=a.hop, segment_s=60.0))
    tab = activity._tables_on(x.device)
    out = {"hours": a.hours, "samples": int(x.numel()), "hop": a.hop, "soundscape_frames": st.total_frames,
           "soundscape_stats_s": timed(lambda: st._frames(stream, tab), a.reps)}
    spec = measurements.MeasureSpec(hop=a.hop)
    for name, seconds in (("one_second", 1), ("one_minute", 60)):
        starts = np.arange(0, int(x.numel()), seconds * SR, dtype=np.int64)
        ends = np.minimum(starts + seconds * SR, int(x.numel()))
        rec = np.zeros(len(starts), dtype=np.int64)
        m = measurements.measure_boxes(ws, rec, starts, ends, spec)
        frames, reduce = m._keep[4], m._keep[5]
        leg = {"events": len(starts), "frames": int(m["frame_offsets"][-1]), "runs": int(((m["n_frames"] + 63) // 64).sum()),
               "frames_s": timed(lambda: frames(stream), a.reps), "reduce_s": timed(lambda: reduce(stream), a.reps),
               "whole_call_s": timed(lambda: measurements.measure_boxes(ws, rec, starts, ends, spec), a.reps)}
        for k in ("frames_s", "reduce_s", "whole_call_s"):
            leg[k.replace("_s", "_over_soundscape_stats")] = leg[k] / out["soundscape_stats_s"]
        leg["frames_per_soundscape_frame"] = leg["frames"] / st.total_frames
        out[name] = leg
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "event measurements on synthetic audio (scripts/measure_bench.py)", "result": out}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
