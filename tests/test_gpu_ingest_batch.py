"""Batched ingest on the device: ingest.load_batch / ingest.Collater (avexhip_ingest_batch).

1. every row is BIT-identical to the per-file path (load_audio, then a torch slice / F.pad), the mask to the torch one;
2. the resampled rows sit within the bars tests/test_ingest.py uses against oracle/ingest_oracle.py (2e-6 sinc, 5e-6 resampy);
3. the reference's own Collater (tests/golden/collater.npz) is reproduced exactly, NaN / Inf rows zeroed;
4. a clip's row does not depend on what else is in the batch;
5. bad descriptors are refused before anything is launched.
"""
import ctypes as C
import io
import os
import struct
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _collater_golden as G
from avex_amd import _capi, ingest, synth
from oracle import ingest_oracle as IO

pytestmark = pytest.mark.gpu

T = 1000                                         # not a multiple of 256: the last workgroup of a row is partial
RATES = (16000, 44100, 48000, 22050, 8000, 32000)
FORMATS = (8, 16, 24, 32, 0, 64)
CHANNELS = (1, 2, 3)
# lengths at the target rate and window starts: 1 frame; shorter than one 256-sample chunk; L < T; L == T; L > T from the clip's start;
# L > T with the window touching the clip's end; L > T from an odd interior start (777: a multiple neither of 256 nor of 160 / 320,
# the reduced output rates of the 44.1 and 22.05 kHz plans)
CASES = ("one_frame", "short", "shorter", "equal", "from_start", "to_end", "odd_start")
L_LONG = 1850


def _wav(x, sr, fmt):
    """[frames, channels] float in [-1, 1) -> WAV bytes in the given sample format."""
    if fmt in (0, 64):
        bits = 32 if fmt == 0 else 64
        data = x.astype("<f4" if fmt == 0 else "<f8").tobytes()
        ch = x.shape[1]
        hdr = struct.pack("<HHIIHH", 3, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits)
        return b"RIFF" + struct.pack("<I", 4 + 8 + len(hdr) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(hdr)) + hdr + b"data" + struct.pack("<I", len(data)) + data
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(x.shape[1]); w.setsampwidth(fmt // 8); w.setframerate(sr)
        if fmt == 8:
            w.writeframes(np.clip(x * 128 + 128, 0, 255).astype(np.uint8).tobytes())
        elif fmt == 16:
            w.writeframes((x * 32767).astype("<i2").tobytes())
        elif fmt == 24:
            v = (x * 8388607).astype(np.int32)
            w.writeframes(np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], -1).astype(np.uint8).tobytes())
        else:
            w.writeframes((x * 2147483647).astype("<i4").tobytes())
    return buf.getvalue()


def _frames_for(sr, n_out):
    """The smallest number of frames at `sr` whose 16 kHz resampling (either resampler: both give ceil(frames * 16000 / sr)) has n_out samples."""
    f = max(1, (n_out - 1) * sr // 16000)
    while -(-f * 16000 // sr) < n_out:
        f += 1
    assert -(-f * 16000 // sr) == n_out
    return f


def _sources():
    out = []
    for k in range(len(RATES) * len(CASES)):
        sr, case, fmt = RATES[k // len(CASES)], CASES[k % len(CASES)], FORMATS[k % len(FORMATS)]
        ch = CHANNELS[(k // len(FORMATS) + k) % len(CHANNELS)]
        n_out = {"one_frame": None, "short": None, "shorter": 700, "equal": T}.get(case, L_LONG)
        frames = 1 if case == "one_frame" else 100 if case == "short" else _frames_for(sr, n_out)
        length = -(-frames * 16000 // sr)
        start = {"to_end": length - T, "odd_start": 777}.get(case, 0)
        x = synth.normal(f"ib{k}", (frames, ch), 0.3).astype(np.float32).clip(-0.99, 0.99)
        out.append(dict(data=_wav(x, sr, fmt), sr=sr, fmt=fmt, ch=ch, frames=frames, length=length, start=start, case=case))
    return out


_RS = {}
SINC_KAISER = "sinc_kaiser"                      # not a res_type of the package: the sinc plan under a Kaiser window (Resampler's beta > 0)


def _resampler(sr, res_type):
    if (sr, res_type) not in _RS:
        _RS[sr, res_type] = (ingest.Resampler(sr, 16000, lowpass_filter_width=16, rolloff=0.945, beta=14.77) if res_type == SINC_KAISER
                             else ingest.Resampler(sr, 16000, res_type=res_type))
    return _RS[sr, res_type]


def _per_file(data, res_type):
    """The per-file path: load_audio, or for another res_type its pieces (parse_wav / FlacStream, to_device_mono, Resampler)."""
    if res_type is None:
        return ingest.load_audio(data, 16000)[0]
    raw, sr, ch, code = ingest.parse_wav(data)
    x = ingest.to_device_mono(raw, ch, code)
    return x if sr == 16000 else _resampler(sr, res_type)(x)


def _expect(x, start, target):
    row = x[start:start + target]
    n = row.numel()
    return F.pad(row, (0, target - n)), torch.arange(target, device=x.device) >= n, n


_BATCH = {}


def _batch(res_type):
    """(sources, load_batch's output, the per-file rows and masks) of the crossing batch; computed once per res_type."""
    if res_type not in _BATCH:
        src = _sources()
        # load_batch has no argument for the Kaiser sinc plan: for this one call it finds the per-file path's own plans in its cache
        lent = {(sr, 16000, None): _resampler(sr, res_type) for sr in RATES if sr != 16000} if res_type == SINC_KAISER else {}
        kept = {k: ingest._BATCH_RESAMPLERS.get(k) for k in lent}
        ingest._BATCH_RESAMPLERS.update(lent)
        try:
            got = ingest.load_batch([s["data"] for s in src], 16000, T, starts=[s["start"] for s in src], res_type=None if lent else res_type)
        finally:
            for k, v in kept.items():
                if v is None:
                    del ingest._BATCH_RESAMPLERS[k]
                else:
                    ingest._BATCH_RESAMPLERS[k] = v
        want = [_expect(_per_file(s["data"], res_type), s["start"], T) for s in src]
        _BATCH[res_type] = (src, got, want)
    return _BATCH[res_type]


@pytest.mark.parametrize("res_type", [None, "kaiser_best", SINC_KAISER])
def test_rows_are_bit_identical_to_the_per_file_path(built_lib, res_type):
    src, (wav, mask, lengths), want = _batch(res_type)
    assert wav.shape == mask.shape == (len(src), T) and wav.dtype == torch.float32 and mask.dtype == torch.bool and wav.is_cuda and mask.is_cuda
    assert lengths.dtype == torch.int64 and lengths.tolist() == [n for _, _, n in want]
    assert {s["case"]: n for s, (_, _, n) in zip(src, want) if s["sr"] == 44100} == {
        "one_frame": 1, "short": 37, "shorter": 700, "equal": T, "from_start": T, "to_end": T, "odd_start": T}
    for b, (s, (row, m, _)) in enumerate(zip(src, want)):
        assert torch.equal(wav[b], row), (b, s["sr"], s["fmt"], s["ch"], s["case"], float((wav[b] - row).abs().max()))
        assert torch.equal(mask[b], m), (b, s["case"])


@pytest.mark.parametrize("res_type,bar", [(None, 2e-6), ("kaiser_best", 5e-6)])
def test_rows_match_the_oracle(built_lib, res_type, bar):
    """The bars of test_device_resampler_matches_oracle / test_device_librosa_resampler_matches_oracle, on clips of the same amplitude."""
    src, (wav, _, lengths), _ = _batch(res_type)
    got = wav.cpu().numpy()
    for b, s in enumerate(src):
        if s["sr"] == 16000:
            continue
        raw, sr, ch, code = ingest.parse_wav(s["data"])
        mono = IO.pcm_to_mono(raw, ch, code)
        ref = IO.resample(mono, sr, 16000) if res_type is None else IO.resample_librosa(mono, sr, 16000)
        assert ref.shape == (s["length"],)
        n = int(lengths[b])
        err = np.abs(got[b, :n] - ref[s["start"]:s["start"] + n]).max()
        assert err < bar, (b, s["sr"], s["fmt"], s["case"], err)
        assert not got[b, n:].any()


def test_single_item_batches_and_longest_item_padding(built_lib):
    src, _, want = _batch(None)
    for b in (9, 12, 20):                        # 44.1 kHz shorter / to_end, 48 kHz odd_start
        wav, mask, lengths = ingest.load_batch([src[b]["data"]], 16000, T, starts=[src[b]["start"]])
        assert wav.shape == (1, T) and torch.equal(wav[0], want[b][0]) and torch.equal(mask[0], want[b][1]) and lengths.tolist() == [want[b][2]]
    pick = [0, 9, 2, 12]                         # target_len=None: padded to the longest resampled item, nothing cropped
    wav, mask, lengths = ingest.load_batch([src[b]["data"] for b in pick])
    assert wav.shape == (4, max(src[b]["length"] for b in pick)) and lengths.tolist() == [src[b]["length"] for b in pick]
    for r, b in enumerate(pick):
        row, m, _ = _expect(_per_file(src[b]["data"], None), 0, wav.shape[1])
        assert torch.equal(wav[r], row) and torch.equal(mask[r], m)


def test_flac_paths_arrays_and_windows(built_lib, tmp_path):
    """FLAC streams are decoded straight into the packed buffer; a path, bytes and an array ride in the same batch; center windows
    and a dataset limit cut what the per-file path followed by the same slice gives."""
    import _flac_enc as E
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac", "xenocanto_XC564654.flac")
    pcm, fsr, bps, bs, plan = E.cases()["three_channels_24bit"]
    enc = E.encode(pcm, fsr, bps, bs, plan)
    src, _, _ = _batch(None)
    path = tmp_path / "clip.wav"
    path.write_bytes(src[11]["data"])             # 44.1 kHz, from_start
    arr = synth.normal("ibarr", (2, 1500), 0.3).astype(np.float32)
    sources = [fixture, enc, str(path), arr, torch.from_numpy(arr[0].astype(np.float64))]
    full = [ingest.load_audio(fixture, 16000)[0], ingest.load_audio(enc, 16000)[0], ingest.load_audio(str(path), 16000)[0],
            ingest.to_device_mono(np.ascontiguousarray(arr.T), 2, 0), ingest.to_device_mono(arr[0].astype(np.float64), 1, 64)]
    assert fsr == 48000 and full[0].numel() == 386361
    starts = [123457, 0, 300, 499, 1]
    wav, mask, lengths = ingest.load_batch(sources, 16000, T, starts=starts)
    for r, (x, s0) in enumerate(zip(full, starts)):
        row, m, n = _expect(x, s0, T)
        assert torch.equal(wav[r], row) and torch.equal(mask[r], m) and int(lengths[r]) == n, r
    wav, mask, lengths = ingest.load_batch(sources, 16000, 600, window_selection="center", dataset_max_len=1200)
    for r, x in enumerate(full):
        L = x.numel()
        s0 = (L - 1200) // 2 + 300 if L > 1200 else max(0, (L - 600) // 2)
        row, m, n = _expect(x, s0, 600)
        assert torch.equal(wav[r], row) and torch.equal(mask[r], m) and int(lengths[r]) == n, r


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_collater_reproduces_the_reference(built_lib, name):
    c = G.cases()[name]
    torch.manual_seed(c["seed"])
    out = ingest.Collater(**c["kwargs"])(c["items"])
    assert set(out) == {"raw_wav", "padding_mask", "label", "text_label"} and out["text_label"] == []
    assert out["raw_wav"].is_cuda and out["raw_wav"].dtype == torch.float32 and out["padding_mask"].dtype == torch.bool
    assert np.array_equal(out["raw_wav"].cpu().numpy(), c["raw_wav"])
    assert np.array_equal(out["padding_mask"].cpu().numpy(), c["padding_mask"])
    assert np.array_equal(out["label"].cpu().numpy(), c["label"])
    bad = [b for b, it in enumerate(c["items"]) if not np.isfinite(G.audio(it)).all()]
    assert len(bad) == (2 if "limit" in name else 0)
    for b in bad:
        assert not out["raw_wav"][b].any()


def test_collater_takes_files_and_text_labels(built_lib):
    src, _, want = _batch(None)
    col = ingest.Collater(1, 1000, window_selection="start", num_labels=3)
    x = synth.normal("ibcol", (2205, 2), 0.3).astype(np.float32).clip(-0.99, 0.99)
    data = _wav(x, 2205, 16)                      # 1 s at 2 205 Hz -> 1 000 samples at the collater's 1 kHz
    out = col([{"audio": data, "label": 2, "text_label": ["a"]}, {"raw_wav": np.ones(400, np.float32), "label": 0, "text_label": "b"}])
    ref = ingest.Resampler(2205, 1000)(ingest.to_device_mono(*[ingest.parse_wav(data)[i] for i in (0, 2, 3)]))
    assert ref.numel() == 1000 and torch.equal(out["raw_wav"][0], ref) and not out["padding_mask"][0].any()
    assert out["padding_mask"][1].tolist() == [False] * 400 + [True] * 600 and out["raw_wav"][1].sum().item() == 400.0
    assert out["label"].tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]] and out["text_label"] == ["a", "b"]


def test_a_row_does_not_depend_on_the_batch_around_it(built_lib):
    src, _, want = _batch(None)
    b = 12                                        # 44.1 kHz, window up to the clip's end
    assert src[b]["sr"] == 44100 and src[b]["case"] == "to_end"
    others = [src[i] for i in (1, 19, 27, 33, 38)]       # other rates, formats, lengths
    for order in ([src[b]], [src[b]] + others, others + [src[b]], others[:2] + [src[b]] + others[2:]):
        wav, mask, _ = ingest.load_batch([s["data"] for s in order], 16000, T, starts=[s["start"] for s in order])
        r = order.index(src[b])
        assert torch.equal(wav[r], want[b][0]) and torch.equal(mask[r], want[b][1]), len(order)


def test_refusals_launch_nothing(built_lib):
    lib = _capi.lib()
    rs = ingest.Resampler(44100, 16000)
    plans = (C.c_void_p * 1)(rs._h)
    raw = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    wav = torch.full((2, 64), 7.0, device="cuda")
    mask = torch.full((2, 64), 7, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")

    def items(**over):
        it = np.zeros(2, dtype=ingest.ITEM_DTYPE)
        it[0] = (128, 100, 0, 37, 16, 1, 0)       # 100 mono 16-bit frames at 44.1 kHz -> 37 samples
        it[1] = (512, 64, 0, 64, 0, 2, -1)        # 64 stereo float32 frames at the target rate
        for k, v in over.items():
            it[k][0] = v
        return it

    def call(it, B=2, n_plans=1, T_out=64, raw_bytes=4096, ws_bytes=ws.numel()):
        rc = lib.avexhip_ingest_batch(raw.data_ptr(), raw_bytes, it.ctypes.data, raw.data_ptr(), B, plans, n_plans, T_out, wav.data_ptr(), 64, mask.data_ptr(),
                                      ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
        return rc, _capi.last_error()

    need = lib.avexhip_ingest_batch_workspace_bytes(items().ctypes.data, 2, plans, 1, 64)
    assert 0 < need <= ws.numel()
    refused = [call(items(valid=65)), call(items(valid=38)),                                   # valid > T_out; a window past the clip's 37 samples
               call(items(offset=4096 - 192)), call(items(offset=1 << 40)), call(items(offset=132)),      # past the buffer end; misaligned
               call(items(), raw_bytes=1000), call(items(plan=1)), call(items(plan=-2)), call(items(), n_plans=0),
               call(items(sample_format=12)), call(items(channels=0)), call(items(frames=0)),
               call(items(), B=0), call(np.zeros(65536, dtype=ingest.ITEM_DTYPE), B=65536)]
    for rc, msg in refused:
        assert rc == -1 and msg.startswith("ingest_batch"), (rc, msg)
    assert lib.avexhip_ingest_batch_workspace_bytes(items(valid=65).ctypes.data, 2, plans, 1, 64) == 0
    rc, msg = call(items(), ws_bytes=need - 1)
    assert rc == -4 and "workspace" in msg
    torch.cuda.synchronize()
    assert bool((wav == 7.0).all()) and bool((mask == 7).all())                                # nothing was launched
    with pytest.raises(ValueError):
        ingest.load_batch([b"OggS" + bytes(64)])
    with pytest.raises(ValueError):
        ingest.load_batch([_wav(np.zeros((10, 1), np.float32), 16000, 16)], 16000, T, starts=[10])
    raw[:80] = torch.from_numpy(items().view(np.uint8).copy())                                 # the same call with good descriptors runs
    rc, msg = call(items())
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not wav[0, 37:].any() and mask[0].tolist() == [0] * 37 + [1] * 27 and not mask[1].any() and not wav[1].any()
