#!/usr/bin/env python3
"""Do two builds of libavexhip.so compute the same thing?

    python scripts/ab_outputs.py LIB_A LIB_B [--set forwards|analytics|audio] [--timeout SECONDS]

Runs one fixed set of small forwards (or, with --set analytics, of small calls of the analytics modules) under each library -- a fresh child process per library (AVEX_AMD_LIB), one after the other, each
under its own time limit; the first child that fails ends the run -- and compares every output array with np.array_equal, every
last_profile() name list and every BeatsGraph.nodes.  For refactors of host code (launchers, layer loops): the second library is usually
a build of the parent commit (AVEX_AMD_LIB_SUFFIX=parent python -m avex_amd.build in a worktree of it).

The set takes the smallest shapes that reach every branch of the layer loops and the GEMM / attention dispatch: BEATs at base width with
2 layers at 1 clip (split-K, LayerNorm in the epilogue), 3 clips (128-tile kernels, LayerNorm kernels on the wide products) and 9 clips
(4 464 rows: over the fold threshold), both residual streams, batch-invariant, unpooled and pooled hooks with and without padding, graph
captures, the loop-shape variants of synth.BEATS_VARIANTS, EAT (513 tokens: nine-tile attention + tail), AVES, EfficientNet-B0 behind the
mel plan with taps, the probes on the stack handle, and tests/test_gpu_source_build.py's FORWARD set.  Exit status 0: everything equal.

The analytics set calls the public functions of search, retrieval, examples, clustering (k-means, scores, silhouette), density and activity
on seeded NumPy inputs, at the smallest shapes that reach every shared block of their kernels (block_prims.h, the rank key of f32_tile.h):
tied keys through all eight radix passes, lists deeper than a chunk, the chunked rank sort, relocation through several empty clusters,
floor ranks on tied and NaN energies.  For refactors of those kernels; it finishes in seconds.

The audio set does the same for ingest, recordings, activity and soundscape (the chains of ingest.hip, the frame walk of rec_frames.h):
every sample format, mono and stereo, without a plan and under a Hann sinc, a Kaiser sinc and an interpolating plan, per file and as
batch rows from inside the clip and padded; a float clip with a NaN; two recordings (40 000 and 700 samples, one NaN sample) in one
buffer at bases that are and are not multiples of 4: window statistics, gathers, a select, the activity gate at hops 160 and 512, the
acoustic indices at hops 256 and 512 with segments of several runs and a partial last one; and for measure, regions (the power row of
frame_power.h, the prefix count of prefix_count.h) over the same buffers: measure_boxes of one frame, 64 and 65 frames, banded boxes and
the NaN frames, with and without a noise spectrum; find_regions at hops 128 and 512 under the noise spectrum of spectral_stats;
label_cells of a random mask of 3 000 frames (three blocks of the prefix count).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(out_path: str) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from avex_amd import _capi, synth, kernels as K

    arrays, profiles, nodes = {}, {}, {}

    def keep(tag, out):
        for k in ("features", "pooled"):
            if out.get(k) is not None:
                arrays[f"{tag}.{k}"] = out[k].float().cpu().numpy()
        for i, t in (out.get("hooks") or {}).items():
            arrays[f"{tag}.hook{i}"] = t.float().cpu().numpy()

    def run(tag, enc, fn):
        enc.set_profiling(True)
        keep(tag, fn())
        torch.cuda.synchronize()
        profiles[tag] = [name for name, _, _ in enc.last_profile()]      # stages in order of first appearance
        enc.set_profiling(False)

    # ---- BEATs, base width, 2 layers, 10 s clips ----
    cfg = dict(synth.BEATS_BASE_CFG, encoder_layers=2)
    sd = synth.beats_state_dict(cfg, seed=5)
    wav9 = torch.from_numpy(synth.noise_clips(9, 160000, seed=9)).cuda()
    for residual in ("half", "f32"):
        enc = K.BeatsEncoder(cfg, sd, operand_dtype="f16", residual=residual)
        for n in (1, 3, 9):
            w = wav9[:n]
            run(f"beats.{residual}.{n}", enc, lambda: enc.forward(w, want_features=True, want_pooled=True))
            run(f"beats.{residual}.{n}.pooled_only", enc, lambda: enc.forward(w, want_features=False, want_pooled=True))
        Tt = enc.num_tokens(160000)
        pad = torch.zeros((9, Tt), dtype=torch.uint8)
        pad[1::2, Tt // 2:] = 1      # every second clip half padding
        run(f"beats.{residual}.9.hooks", enc, lambda: enc.forward(wav9, hook_layers=[0, 1, 2], want_features=False))
        for mode in ("mean", "max", "cls_token"):
            run(f"beats.{residual}.9.{mode}", enc, lambda: enc.forward(wav9, hook_layers=[0, 1, 2], hook_pooled=mode, want_features=False, want_pooled=True))
            run(f"beats.{residual}.9.{mode}.pad", enc, lambda: enc.forward(wav9, hook_layers=[0, 1, 2], hook_pooled=mode, want_features=False, want_pooled=True, frame_pad=pad.cuda()))
        for n in (1, 9):
            g = enc.capture(n, 160000, want_features=True, want_pooled=True)
            g.wav.copy_(wav9[:n])
            g.replay()
            torch.cuda.synchronize()
            nodes[f"beats.{residual}.{n}"] = g.nodes
            keep(f"beats.{residual}.{n}.graph", dict(features=g.features, pooled=g.pooled))
            g.close()
        enc.close()
    inv = K.BeatsEncoder(cfg, sd, operand_dtype="f16", residual="half", batch_invariant=True)
    run("beats.invariant.9", inv, lambda: inv.forward(wav9, want_features=True, want_pooled=True))
    run("beats.invariant.9.pooled_only", inv, lambda: inv.forward(wav9, want_features=False, want_pooled=True))
    for mode in ("mean", "max", "cls_token"):
        run(f"beats.invariant.9.{mode}", inv, lambda: inv.forward(wav9, hook_layers=[0, 1, 2], hook_pooled=mode, want_features=False))
    inv.close()
    # ---- the loop shapes: pre-LN, no post_extract_proj, GLU, identity activation ----
    for name in ("preln_relu_convbias", "preln_tanh_nopost", "postln_glu_nogate", "postln_linear"):
        vcfg = synth.BEATS_VARIANTS[name]
        for residual in ("half", "f32"):
            v = K.BeatsEncoder(vcfg, synth.beats_state_dict(vcfg, seed=3), operand_dtype="f16", residual=residual)
            run(f"variant.{name}.{residual}", v, lambda: v.forward(wav9[:2], hook_layers=[1, 2], want_features=True, want_pooled=True))
            run(f"variant.{name}.{residual}.pooled_only", v, lambda: v.forward(wav9[:2], want_features=False, want_pooled=True))
            v.close()
    # ---- EAT: 513 tokens ----
    from avex_amd.eat_encoder import EatEncoder
    ecfg = dict(synth.EAT_BASE_CFG, depth=2)
    eat = EatEncoder(ecfg, synth.eat_state_dict(ecfg), operand_dtype="f16")
    ew = torch.from_numpy(synth.noise_clips(3, 48000, seed=10)).cuda()
    run("eat.cls", eat, lambda: eat.forward(ew, hook_layers=[0, 1], pooling="cls"))
    run("eat.cls.pooled_only", eat, lambda: eat.forward(ew, want_features=False, pooling="cls"))
    run("eat.mean", eat, lambda: eat.forward(ew, want_features=False, pooling="mean", hook_layers=[1], hook_pooled=True))
    eat.close()
    # ---- AVES ----
    from avex_amd.aves_encoder import AvesEncoder
    acfg = dict(synth.AVES_BASE_CFG, encoder_num_layers=2)
    aves = AvesEncoder(acfg, synth.aves_state_dict(acfg))
    aw = torch.from_numpy(synth.noise_clips(3, 32000, seed=12)).cuda()
    run("aves", aves, lambda: aves.forward(aw, hook_layers=[0, 1], want_features=True, want_pooled=True))
    run("aves.pooled_only", aves, lambda: aves.forward(aw, want_features=False, want_pooled=True))
    aves.close()
    # ---- EfficientNet-B0 behind the mel plan ----
    from avex_amd.effnet_encoder import EfficientNetB0Encoder
    eff = EfficientNetB0Encoder(synth.effnet_b0_state_dict())
    mel = K.MelspecPlan(n_fft=800, hop_length=160, n_mels=128, normalize=True)(torch.from_numpy(synth.noise_clips(3, 64000, seed=11)).cuda())
    run("effnet", eff, lambda: eff.forward(mel, hook_layers=eff.tap_names(), want_features=True, want_pooled=True))
    eff.close()
    # ---- probes on the stack handle: attention-only blocks (F = 0) and head widths other than 64 ----
    from avex_amd import probes as P
    gen = torch.Generator().manual_seed(4)
    seqs = [torch.randn(5, 24, 128, generator=gen).cuda() for _ in range(3)]
    torch.manual_seed(7)
    att = P.AttentionProbe(None, [], 37, device="cuda", feature_mode=True, input_dim=[(24, 128)] * 3, aggregation="none", num_heads=4, num_layers=2,
                           dropout_rate=0.0, max_sequence_length=64, use_positional_encoding=True).eval()
    arrays["probe.attention"] = att(seqs).float().cpu().numpy()
    tr = P.TransformerProbe(None, [], 19, device="cuda", feature_mode=True, input_dim=[(24, 128)] * 3, aggregation="none", num_heads=4, attention_dim=192,
                            num_layers=2, dropout_rate=0.0, max_sequence_length=64, use_positional_encoding=True).eval()
    arrays["probe.transformer"] = tr(seqs).float().cpu().numpy()
    # ---- tests/test_gpu_source_build.py's set ----
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_source_build as sb
    fd, side = tempfile.mkstemp(suffix=".npz")
    os.close(fd)
    exec(compile(sb.FORWARD.format(root=ROOT, out=side), "FORWARD", "exec"), {"__name__": "forward_set"})
    with np.load(side) as z:
        for k in z.files:
            if k != "lib":
                arrays[f"source_build.{k}"] = z[k]
    os.remove(side)
    torch.cuda.synchronize()
    np.savez(out_path, **arrays)
    with open(out_path + ".json", "w") as f:
        json.dump(dict(lib=_capi.LIB_PATH, profiles=profiles, nodes=nodes), f)


def child_analytics(out_path: str) -> None:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _retrieval_ref as RR
    from avex_amd import _capi, activity, clustering, density, examples, recordings, retrieval, search

    arrays = {}

    def keep(tag, out):
        for k, v in (out.items() if isinstance(out, dict) else enumerate(out)):
            if isinstance(v, torch.Tensor):
                arrays[f"{tag}.{k}"] = v.cpu().numpy()
            elif isinstance(v, (bool, int, float, str, np.generic, np.ndarray)):
                arrays[f"{tag}.{k}"] = np.asarray(v)
            elif v is not None:                                  # nothing a function returns goes uncompared without notice
                raise TypeError(f"{tag}.{k}: a {type(v).__name__} is neither a tensor, an array nor a scalar")

    rng = np.random.default_rng(23)
    # ---- search: 300 rows in chunks of 128 (three merges); rows 100..163 are row 7 again: keys that tie in their high word ----
    rows = rng.standard_normal((300, 40)).astype(np.float32)
    rows[100:164] = rows[7]
    q = rng.standard_normal((5, 40)).astype(np.float32)
    q[0] = rows[7]
    ix = search.EmbeddingIndex(40, metric="cosine", chunk_rows=128)
    start = (np.arange(300) % 50) * 0.25
    ix.add(rows, recording=(np.arange(300) // 50).astype(np.int32), start_s=start, end_s=start + 1.0)
    keep("search.k8.nms", ix.search(q, 8, nms=0.5))
    keep("search.k8", ix.search(q, 8))
    keep("search.k300", ix.search(q, 300))                       # deeper than a chunk: every key survives (total <= kp)
    # ---- retrieval: self-set and cross-set, and the chunk-threshold shape (chunked sort, count_below) ----
    lab = rng.integers(0, 4, size=300)
    keep("retrieval.self", retrieval.retrieval_stats(rows, lab, k=5))
    keep("retrieval.cross", retrieval.retrieval_stats(q, lab[:5], rows, lab, k=5))
    cq, cqi, cdb, cdi = RR.chunked_case(n0=16385, d=8, per_class=1)
    keep("retrieval.chunked", retrieval.retrieval_stats(cq, cqi, cdb, cdi, k=5))
    # ---- examples: classes of 5, 17 and 130 rows (one and two tiles) and a background, margin mode, nearest ----
    bank = examples.ExampleBank(40)
    blab = np.concatenate([np.repeat(np.arange(3), (5, 17, 130)), np.full(11, -1)])
    order = rng.permutation(len(blab))
    bank.add(rng.standard_normal((len(blab), 40)).astype(np.float32), blab[order])
    eq = rng.standard_normal((9, 40)).astype(np.float32)
    keep("examples.margin", bank.score(eq, top_m=3, mode="margin", return_nearest=True))
    keep("examples.similarity", bank.score(eq, top_m=3, return_nearest=True))
    # ---- clustering: 3 distinct points for 12 clusters (relocation through several empties), the scores of two label vectors ----
    pts = rng.standard_normal((3, 16)).astype(np.float32)
    keep("kmeans", clustering.kmeans(pts[rng.integers(0, 3, size=200)], 12, n_init=2))
    keep("clustering_scores", clustering.clustering_scores(rng.integers(0, 5, size=200), rng.integers(0, 7, size=200)))
    # ---- density, silhouette ----
    dx = (rng.standard_normal((6, 33))[rng.integers(0, 6, size=257)] + 0.05 * rng.standard_normal((257, 33))).astype(np.float32)
    keep("dbscan.cosine", density.dbscan(dx, 0.01, 4, metric="cosine"))
    keep("dbscan.euclidean", density.dbscan(dx, 0.6, 4, metric="euclidean"))
    sx, sl = rng.standard_normal((200, 16)).astype(np.float32), rng.integers(0, 5, size=200)
    for metric in ("euclidean", "cosine"):
        arrays[f"silhouette.{metric}.samples"] = clustering.silhouette_samples(sx, sl, metric=metric).cpu().numpy()
        arrays[f"silhouette.{metric}.score"] = np.asarray(clustering.silhouette_score(sx, sl, metric=metric))
    # ---- activity: 3 s at 16 kHz with a silent second (ties at key 0) and one NaN sample; the floor at three ranks ----
    wav = (0.01 * rng.standard_normal(48000)).astype(np.float32)
    wav[16000:32000] = 0.0
    wav[40000] = np.nan
    ws = recordings.RecordingWindows([torch.from_numpy(wav).cuda()], 16000, 8000, 4000)
    for pct in (0.0, 20.0, 100.0):
        act = activity.band_activity(ws, activity.ActivityGate([(500, 2000), (2000, 8000)], hop=160, floor_percentile=pct))
        keep(f"activity.p{pct:g}", dict(frame_energy=act.frame_energy, floor=act.floor, nonfinite=act.nonfinite_frames, n_frames=act.n_frames,
                                        active=act.active_frames, max_energy=act.max_energy, kept=act.select()))
    torch.cuda.synchronize()
    np.savez(out_path, **arrays)
    with open(out_path + ".json", "w") as f:
        json.dump(dict(lib=_capi.LIB_PATH, profiles={}, nodes={}), f)


def child_audio(out_path: str) -> None:
    import numpy as np
    import torch
    import struct
    sys.path.insert(0, ROOT)
    from avex_amd import _capi, activity, ingest, measurements, recordings, regions, soundscape
    from avex_amd._capi import check, lib

    def _wav(x, sr, fmt):
        """[frames, channels] float in [-1, 1) -> RIFF/WAVE bytes: 8 / 16 / 24 / 32-bit integer PCM, 0 = float32, 64 = float64."""
        bits = {0: 32, 64: 64}.get(fmt, fmt)
        if fmt in (0, 64):
            data = x.astype("<f4" if fmt == 0 else "<f8").tobytes()
        elif fmt == 8:
            data = np.clip(x * 128 + 128, 0, 255).astype(np.uint8).tobytes()
        elif fmt == 24:
            v = (x * 8388607).astype(np.int32)
            data = np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], -1).astype(np.uint8).tobytes()
        else:
            data = (x * (2 ** (fmt - 1) - 1)).astype("<i2" if fmt == 16 else "<i4").tobytes()
        ch = x.shape[1]
        hdr = struct.pack("<HHIIHH", 3 if fmt in (0, 64) else 1, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits)
        return b"RIFF" + struct.pack("<I", 20 + len(hdr) + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(hdr)) + hdr + b"data" + struct.pack("<I", len(data)) + data

    arrays = {}
    rng = np.random.default_rng(29)
    # ---- ingest: every sample format, mono and stereo, under the four kinds of plan; per file and in a batch ----
    kaiser = ingest.Resampler(22050, 16000, lowpass_filter_width=16, rolloff=0.945, beta=14.77)
    interp = ingest.Resampler(32000, 16000, res_type="kaiser_best")
    T = 1000
    for plan, sr, res_type in (("none", 16000, None), ("hann", 44100, None), ("kaiser", 22050, None), ("interp", 32000, "kaiser_best")):
        tags, clips, starts = [], [], []
        for fmt in (8, 16, 24, 32, 0, 64):
            for ch in (1, 2):
                frames = int(rng.integers(3000, 9001))
                data = _wav(rng.uniform(-0.9, 0.9, size=(frames, ch)).astype(np.float32), sr, fmt)
                if plan in ("none", "hann"):
                    x = ingest.load_audio(data, 16000)[0]
                else:                                            # load_audio's pieces, under a plan it does not make
                    raw, _, _, code = ingest.parse_wav(data)
                    x = (kaiser if plan == "kaiser" else interp)(ingest.to_device_mono(raw, ch, code))
                arrays[f"ingest.{plan}.f{fmt}.c{ch}.file"] = x.cpu().numpy()
                tags += [f"ingest.{plan}.f{fmt}.c{ch}"] * 2
                clips += [data, data]
                starts += [333, x.numel() - 400]                 # a window from inside the clip, and one the clip's end cuts short: padding
        if plan == "kaiser":                                     # load_batch has no argument for a Kaiser sinc plan: it finds this one, for this call
            ingest._BATCH_RESAMPLERS[sr, 16000, None] = kaiser
        wav, mask, lengths = ingest.load_batch(clips, 16000, T, starts=starts, res_type=res_type)
        if plan == "kaiser":
            del ingest._BATCH_RESAMPLERS[sr, 16000, None]
        for b, tag in enumerate(tags):
            arrays[f"{tag}.batch{b % 2}"] = np.concatenate([wav[b].cpu().numpy(), mask[b].cpu().numpy().astype(np.float32), [float(lengths[b])]])
    bad = rng.uniform(-0.5, 0.5, size=(2, 4000)).astype(np.float32)
    bad[1, 1234] = np.nan                                        # a float clip that holds a NaN: a NaN per file, a zero row in the batch
    arrays["ingest.nan.file"] = ingest.to_device_mono(np.ascontiguousarray(bad.T), 2, 0).cpu().numpy()
    wav, mask, _ = ingest.load_batch([bad, bad[0]], 16000, T)
    arrays["ingest.nan.batch"], arrays["ingest.nan.mask"] = wav.cpu().numpy(), mask.cpu().numpy()

    # ---- recordings of 40 000 and 700 samples in one buffer, one NaN sample; as RecordingWindows lays them out (bases 0 and 40 000) and
    # one sample further (odd bases: stage_span's lead-in, the single loads of windows.hip) ----
    a = (0.05 * rng.standard_normal(40000)).astype(np.float32)
    a[8000:12000] = 0.0
    a[39001] = np.nan                                            # in the last segment at both hops
    b = (0.05 * rng.standard_normal(700)).astype(np.float32)
    ws0 = recordings.RecordingWindows([torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], 16000, 8000, 4000)
    ws1 = recordings.RecordingWindows([torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], 16000, 8000, 4000)
    ws1.wav = torch.cat([torch.zeros(1, device="cuda"), ws1.wav])
    ws1._table["base"] += 1
    ws1._table_pinned = torch.from_numpy(ws1._table.view(np.uint8).reshape(-1)).pin_memory()
    ws1._table_dev = ws1._table_pinned.cuda()
    check(lib().avexhip_window_stats(ws1.wav.data_ptr(), ws1.wav.numel(), ws1._table.ctypes.data, ws1._table_dev.data_ptr(), ws1.n_windows, ws1.window_len,
                                     ws1.energy.data_ptr(), ws1.peak.data_ptr(), torch.cuda.current_stream().cuda_stream), "window_stats")
    for tag, ws in (("rec.base0", ws0), ("rec.base1", ws1)):
        rows, mask = ws.batch(torch.arange(ws.n_windows - 1, -1, -1))
        arrays.update({f"{tag}.energy": ws.energy.cpu().numpy(), f"{tag}.peak": ws.peak.cpu().numpy(), f"{tag}.rows": rows.cpu().numpy(),
                       f"{tag}.mask": mask.cpu().numpy(), f"{tag}.range": ws.batch(1, 3)[0].cpu().numpy(), f"{tag}.kept": ws.select(-40.0, -30.0).cpu().numpy()})
        for hop in (160, 512):                                   # the span of a workgroup at its shortest and its longest
            act = activity.band_activity(ws, activity.ActivityGate([(500, 2000), (2000, 8000)], hop=hop))
            for k in ("frame_energy", "floor", "nonfinite_frames", "n_frames", "active_frames", "max_energy"):
                arrays[f"{tag}.activity.h{hop}.{k}"] = getattr(act, k).cpu().numpy()
            arrays[f"{tag}.activity.h{hop}.kept"] = act.select().cpu().numpy()
        for hop in (256, 512):                                   # 2.24 s: 140 / 70 frames a segment (three / two runs), a partial last segment
            ix = soundscape.acoustic_indices(ws, soundscape.IndexSpec(hop=hop, segment_s=2.24))
            for k in ("mean_power", "mean_amplitude", "abs_diff", "count_above", "frame_power", "nonfinite_frames"):
                arrays[f"{tag}.soundscape.h{hop}.{k}"] = getattr(ix.stats, k).cpu().numpy()
            arrays[f"{tag}.soundscape.h{hop}.indices"] = ix.values.cpu().numpy()
        # boxes of recording 0 at hop 256: one frame, 64 and 65 frames (a run and a run plus one), two banded ones, the frames around the
        # NaN sample; the one frame of recording 1
        rec, s0, s1 = [0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 1000, 20000, 38400, 0], [512, 16640, 16896, 9000, 30001, 40000, 700]
        bins = [[0, 257], [0, 257], [0, 257], [40, 120], [255, 257], [0, 257], [3, 200]]
        noise = measurements.noise_spectrum(soundscape.spectral_stats(ws, soundscape.IndexSpec(hop=256, segment_s=0.5)))
        for name, np_ in (("plain", None), ("noise", noise)):
            m = measurements.measure_boxes(ws, rec, s0, s1, measurements.MeasureSpec(hop=256), noise_power=np_, bins=bins)
            arrays.update({f"{tag}.measure.{name}.{k}": v.cpu().numpy() for k, v in m.items()})
        for hop in (128, 512):
            noise = measurements.noise_spectrum(soundscape.spectral_stats(ws, soundscape.IndexSpec(hop=hop, segment_s=0.5)))
            r = regions.find_regions(ws, regions.RegionSpec(hop=hop, snr_db=6.0, min_db=-80.0), noise_power=noise)
            arrays.update({f"{tag}.regions.h{hop}.{k}": v.cpu().numpy() for k, v in r.items()})
            arrays.update({f"{tag}.regions.h{hop}.{k}": getattr(r, k).cpu().numpy() for k in ("cells", "nonfinite_frames", "n_found")})
    # ---- label_cells: 3 000 frames of a fixed random mask, more than two blocks of the prefix count, as two recordings ----
    r = regions.label_cells(torch.from_numpy(rng.random((3000, 257)) < 0.01).cuda(), [1900, 1100], (2, 2), min_cells=2)
    arrays.update({f"label_cells.{k}": v.cpu().numpy() for k, v in r.items()})
    arrays.update({f"label_cells.{k}": getattr(r, k).cpu().numpy() for k in ("cells", "n_found")})
    torch.cuda.synchronize()
    np.savez(out_path, **arrays)
    with open(out_path + ".json", "w") as f:
        json.dump(dict(lib=_capi.LIB_PATH, profiles={}, nodes={}), f)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--set", choices=("forwards", "analytics", "audio"), default="forwards", help="which fixed set to run")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", metavar="OUT", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        {"forwards": child, "analytics": child_analytics, "audio": child_audio}[a.set](a.child)
        return 0
    import numpy as np
    res = []
    with tempfile.TemporaryDirectory() as td:
        for tag, lib in (("a", a.lib_a), ("b", a.lib_b)):
            lib = os.path.abspath(lib)
            out = os.path.join(td, tag + ".npz")
            env = dict(os.environ, AVEX_AMD_LIB=lib)
            env.pop("AVEX_AMD_LIB_SUFFIX", None)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), lib, lib, "--set", a.set, "--child", out], env=env, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"ab_outputs: the run under {lib} did not finish in {a.timeout} s; stopping")
                return 3
            if r.returncode != 0:
                print(f"ab_outputs: the run under {lib} failed with status {r.returncode}; stopping")
                return 2
            with open(out + ".json") as f:
                meta = json.load(f)
            assert meta["lib"] == lib, (meta["lib"], lib)
            with np.load(out) as z:
                res.append((dict(z), meta))
    (xa, ma), (xb, mb) = res
    bad = 0
    if sorted(xa) != sorted(xb):
        print("ab_outputs: the two runs returned different sets of arrays")
        bad += 1
    for k in sorted(set(xa) & set(xb)):
        if xa[k].shape != xb[k].shape or not np.array_equal(xa[k], xb[k], equal_nan=True):
            d = np.abs(xa[k].astype(np.float64) - xb[k].astype(np.float64)).max() if xa[k].shape == xb[k].shape else float("nan")
            print(f"DIFF array {k}: shapes {xa[k].shape} {xb[k].shape}, max |a - b| = {d:.3g}")
            bad += 1
        elif not np.isfinite(xa[k]).all():
            print(f"note: {k} holds non-finite values (equal in both)")
    for kind in ("profiles", "nodes"):
        for k in sorted(set(ma[kind]) | set(mb[kind])):
            if ma[kind].get(k) != mb[kind].get(k):
                print(f"DIFF {kind} {k}:\n  a: {ma[kind].get(k)}\n  b: {mb[kind].get(k)}")
                bad += 1
    print(f"ab_outputs: {len(xa)} arrays, {len(ma['profiles'])} profile name lists, {len(ma['nodes'])} graph node counts compared: "
          + ("all equal" if not bad else f"{bad} differ"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
