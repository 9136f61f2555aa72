"""Audio ingest for the embedding path: file -> mono float32 at the model's sample rate, decoded and resampled on the GPU
(SURVEY.md section 8, row f4).

What the reference does on the host before a clip reaches a model: read the file (``soundfile`` / ``torchaudio.load``), average the
channels (``noise_wav.mean(dim=0)``, avex/data/augmentations.py:269-271; ``audio_stereo_to_mono(..., "average")``,
avex/data/birdset_train_splits.py:184-186) and resample when the rate differs (``torchaudio.transforms.Resample(sr, self.sr)``,
augmentations.py:274-276; ``librosa.resample(..., res_type="kaiser_best")``, birdset_train_splits.py:190-196).  Here the host only
parses the container: the raw PCM bytes go to the device as they are and ``avexhip_pcm_to_mono_f32`` / ``avexhip_resample_forward``
do the rest (a 44.1 kHz stereo minute is 10 MB over PCIe instead of 3.8 MB of finished floats, but no host core touches a sample).

Containers: RIFF/WAVE with integer PCM (8 / 16 / 24 / 32 bit) or IEEE float (32 / 64 bit), incl. WAVE_FORMAT_EXTENSIBLE, and -- round 3 --
FLAC (:class:`FlacStream`: the bitstream is parsed on the host, the predictors run on the device, bit-exact against the MD5 every
stream carries); lossy codecs (MP3, OGG Vorbis) need a codec library that neither machine has and raise ``ValueError`` -- decode
those with the reference's reader and hand the array to :func:`to_device_mono`.  The resampler is torchaudio's algorithm (Hann-windowed sinc); librosa's ``kaiser_best``
filter is a different low-pass design and is NOT reproduced sample for sample (PARITY UNPINNED for both: neither library is
installed; checker = oracle/ingest_oracle.py).

:func:`load_batch` / :class:`Collater` turn a whole batch of files into the padded ``[B, T]`` batch and padding mask of the reference's
``Collater`` (avex/data/dataset.py:256-399) in one copy and a fixed number of launches (``avexhip_ingest_batch``), each row bit-identical
to :func:`load_audio` followed by a slice / pad.
"""
from __future__ import annotations

import os
import struct
import random
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi
from ._capi import AvexHipError, check, lib

__all__ = ["parse_wav", "FlacStream", "Resampler", "to_device_mono", "load_audio", "load_batch", "Collater"]


def parse_wav(path_or_bytes: Union[str, bytes]) -> Tuple[np.ndarray, int, int, int]:
    """``(raw uint8 samples, sample_rate, channels, sample_format)`` of a RIFF/WAVE file; ``sample_format`` as avexhip_pcm_to_mono_f32
    takes it (8 / 16 / 24 / 32 integer PCM, 0 float32, 64 float64).  No sample is converted on the host."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file (only PCM / float WAV is decoded here)")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        body = data[pos + 8: pos + 8 + size]
        if cid == b"fmt ":
            if len(body) < 16:
                raise ValueError(f"WAVE fmt chunk of {len(body)} bytes (at least 16 expected)")
            tag, ch, sr, _br, block_align, bits = struct.unpack_from("<HHIIHH", body, 0)
            if tag == 0xFFFE:                                           # WAVE_FORMAT_EXTENSIBLE: the real tag is in the sub-format GUID
                if len(body) < 26:
                    raise ValueError(f"WAVE_FORMAT_EXTENSIBLE fmt chunk of {len(body)} bytes (at least 26 expected)")
                tag = struct.unpack_from("<H", body, 24)[0]
            if ch <= 0 or sr <= 0:
                raise ValueError(f"WAVE fmt chunk with {ch} channels at {sr} Hz")
            if bits % 8 or block_align != ch * bits // 8:
                raise ValueError(f"WAVE fmt chunk: block_align {block_align} is not channels x bytes per sample ({ch} x {bits} bits); "
                                 "padded containers are not decoded here")
            fmt = (tag, ch, sr, bits)
        elif cid == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise ValueError("WAVE file without a fmt or data chunk")
    tag, ch, sr, bits = fmt
    if tag == 1 and bits in (8, 16, 24, 32):
        code = bits
    elif tag == 3 and bits in (32, 64):
        code = 0 if bits == 32 else 64
    else:
        raise ValueError(f"unsupported WAVE encoding (format tag {tag}, {bits} bits)")
    frame_bytes = ch * bits // 8
    n = len(payload) // frame_bytes                                     # a truncated last frame is dropped
    return np.frombuffer(payload, dtype=np.uint8, count=n * frame_bytes), sr, ch, code


class FlacStream:
    """A FLAC stream parsed on the host (``avexhip_flac_open``: metadata, frame / subframe headers, Rice-coded residuals, every CRC) and
    decoded on the device (``avexhip_flac_decode_i32``: predictors + inter-channel decorrelation), bit-exact -- the stream's STREAMINFO
    carries the MD5 of its unencoded audio (``md5``).  Raises ``ValueError`` for anything that is not a well-formed FLAC stream."""

    def __init__(self, data: Union[str, bytes]) -> None:
        raw = data if isinstance(data, (bytes, bytearray)) else open(data, "rb").read()
        self._buf = bytes(raw)
        self._h = lib().avexhip_flac_open(self._buf, len(self._buf))
        if not self._h:
            raise ValueError(f"FLAC: {_capi.last_error()}")
        import ctypes as C
        sr, ch, bps, tot, md5 = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), (C.c_uint8 * 16)()
        check(lib().avexhip_flac_info(self._h, C.byref(sr), C.byref(ch), C.byref(bps), C.byref(tot), md5), "flac_info")
        self.sample_rate, self.channels, self.bits_per_sample, self.total_samples, self.md5 = sr.value, ch.value, bps.value, tot.value, bytes(md5)

    def decode(self, device: Optional[torch.device] = None, left_justify: bool = False) -> torch.Tensor:
        """Interleaved ``[total_samples, channels]`` int32 samples on the device (``left_justify``: shifted to 32-bit full scale)."""
        _capi.require_gpu()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            out = torch.empty((self.total_samples, self.channels), dtype=torch.int32, device=dev)
            check(lib().avexhip_flac_decode_i32(self._h, out.data_ptr(), int(left_justify), torch.cuda.current_stream().cuda_stream), "flac_decode_i32")
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().avexhip_flac_close(self._h)
            self._h = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


# resampy's published filters: (num_zeros, precision, rolloff, Kaiser beta)
RESAMPY_FILTERS = {"kaiser_best": (64, 9, 0.9475937167399596, 14.769656459379492),
                   "kaiser_fast": (16, 9, 0.85, 8.555504641634386)}


class Resampler:
    """``torchaudio.transforms.Resample(orig_freq, new_freq)`` on the device (defaults as torchaudio's: ``sinc_interp_hann``,
    ``lowpass_filter_width=6``, ``rolloff=0.99``; ``beta`` > 0 selects the Kaiser window, ``sinc_interp_kaiser``)."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, beta: float = 0.0,
                 res_type: Optional[str] = None, scale: bool = True) -> None:
        """``res_type="kaiser_best"`` selects librosa's resampler instead (``librosa.resample(y, orig_sr=, target_sr=, scale=True,
        res_type="kaiser_best")``, birdset_train_splits.py:190-196 = resampy's interpolating kernel with its published kaiser_best
        filter); ``scale`` is librosa's energy-preserving ``scale`` flag."""
        _capi.require_gpu()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self._h = None
        if self.orig_freq != self.new_freq:
            if res_type is None:
                self._h = lib().avexhip_resample_plan_create(self.orig_freq, self.new_freq, int(lowpass_filter_width), float(rolloff), float(beta))
            elif res_type in RESAMPY_FILTERS:
                nz, prec, ro, kb = RESAMPY_FILTERS[res_type]
                self._h = lib().avexhip_resample_interp_plan_create(self.orig_freq, self.new_freq, nz, prec, ro, kb, int(bool(scale)))
            else:
                raise ValueError(f"res_type {res_type!r}: only {sorted(RESAMPY_FILTERS)} (librosa / resampy) or None (torchaudio sinc) are built")
            if not self._h:
                raise AvexHipError(f"resample_plan_create failed: {_capi.last_error()}")

    def out_length(self, T: int) -> int:
        return T if self._h is None else int(lib().avexhip_resample_out_length(self._h, T))

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError("Resampler takes float32 CUDA tensors ([T] or [B, T])")
        if self._h is None:
            return x
        squeeze = x.dim() == 1
        x2 = (x.unsqueeze(0) if squeeze else x).contiguous()
        B, T = x2.shape
        out = torch.empty((B, self.out_length(T)), dtype=torch.float32, device=x.device)
        check(lib().avexhip_resample_forward(self._h, x2.data_ptr(), B, T, T, out.data_ptr(), out.shape[1], torch.cuda.current_stream().cuda_stream),
              "resample_forward")
        return out[0] if squeeze else out

    def __del__(self) -> None:
        try:
            if getattr(self, "_h", None):
                lib().avexhip_resample_plan_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001
            pass


def to_device_mono(raw: Union[np.ndarray, torch.Tensor], channels: int, sample_format: int, device: Optional[torch.device] = None) -> torch.Tensor:
    """Interleaved samples as the file holds them (uint8 view, or a float32 / int16 / ... array of shape ``[frames, channels]``) -> mono
    float32 ``[frames]`` on the device, channels averaged."""
    _capi.require_gpu()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    if isinstance(raw, np.ndarray):
        a = np.ascontiguousarray(raw)
        t = torch.from_numpy(a if a.flags.writeable else a.copy())      # (views of a bytes object are read-only; torch wants to own writable memory)
    else:
        t = raw
    buf = t.contiguous().view(torch.uint8).reshape(-1)
    width = {8: 1, 16: 2, 24: 3, 32: 4, 0: 4, 64: 8}[sample_format]
    frames = buf.numel() // (width * channels)
    if frames <= 0:
        raise ValueError("no audio frames")
    d = buf.to(dev, non_blocking=True)
    out = torch.empty((frames,), dtype=torch.float32, device=dev)
    check(lib().avexhip_pcm_to_mono_f32(d.data_ptr(), sample_format, channels, frames, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "pcm_to_mono_f32")
    return out


_RESAMPLERS: Dict[Tuple[int, int], Resampler] = {}


def load_audio(path_or_bytes: Union[str, bytes], target_sr: Optional[int] = 16000, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, int]:
    """WAV or FLAC file -> ``(mono float32 [T] on the device, sample_rate)``; resampled to ``target_sr`` when it differs (``None``: keep)."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if data[:4] == b"fLaC":
        fl = FlacStream(data)
        pcm = fl.decode(device, left_justify=True)          # int32 at 32-bit full scale: normalised like 32-bit PCM (soundfile's float32 reading)
        x, sr = to_device_mono(pcm, fl.channels, 32, device), fl.sample_rate
        fl.close()
    else:
        raw, sr, ch, code = parse_wav(data)
        x = to_device_mono(raw, ch, code, device)
    if target_sr is not None and sr != target_sr:
        key = (sr, int(target_sr))
        if key not in _RESAMPLERS:
            _RESAMPLERS[key] = Resampler(sr, int(target_sr))
        x, sr = _RESAMPLERS[key](x), int(target_sr)
    return x, sr


# ------------------------------------------------------------------------------------------------------------------------
# Batched ingest: files -> the padded batch a model takes (avexhip_ingest_batch), what the reference's Collater builds on the host
# (avex/data/dataset.py:256-399 on avex/data/audio_utils.py:16-73).  The host parses containers and chooses the windows; every sample is
# decoded, averaged, resampled, cropped and padded on the device, from one packed buffer that crosses PCIe in one copy.
# ------------------------------------------------------------------------------------------------------------------------
WINDOW_SELECTIONS = ("random", "center", "start")
# avexhip_ingest_item, field for field
ITEM_DTYPE = np.dtype([("offset", "<i8"), ("frames", "<i8"), ("start", "<i8"), ("valid", "<i4"), ("sample_format", "<i4"), ("channels", "<i4"),
                       ("plan", "<i4")])
_SAMPLE_BYTES = {8: 1, 16: 2, 24: 3, 32: 4, 0: 4, 64: 8}


class _Entry:
    """One source after its container was parsed: the payload as the file holds it (or the FLAC stream that will be decoded into the
    packed buffer), its rate, layout and length."""
    __slots__ = ("payload", "flac", "sr", "channels", "fmt", "frames")

    def __init__(self, payload, flac, sr, channels, fmt, frames):
        self.payload, self.flac, self.sr, self.channels, self.fmt, self.frames = payload, flac, int(sr), int(channels), int(fmt), int(frames)
        if self.frames <= 0:
            raise ValueError("no audio frames")

    @property
    def nbytes(self) -> int:
        return self.frames * self.channels * _SAMPLE_BYTES[self.fmt]


def _open_source(src: Any, array_sr: int) -> _Entry:
    """A path or bytes (WAV / FLAC), or a ``(T,)`` / ``(C, T)`` float array or tensor taken to be at ``array_sr``."""
    if isinstance(src, (str, os.PathLike, bytes, bytearray)):
        data = bytes(src) if isinstance(src, (bytes, bytearray)) else open(src, "rb").read()
        if data[:4] == b"fLaC":
            fl = FlacStream(data)
            return _Entry(None, fl, fl.sample_rate, fl.channels, 32, fl.total_samples)      # decoded left-justified: 32-bit full scale
        raw, sr, ch, code = parse_wav(data)
        return _Entry(raw, None, sr, ch, code, raw.size // (ch * _SAMPLE_BYTES[code]))
    a = src.detach().cpu().numpy() if isinstance(src, torch.Tensor) else np.asarray(src)
    if a.ndim not in (1, 2):
        raise ValueError(f"audio array of shape {a.shape}: (T,) or (C, T) expected")
    a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
    ch = 1 if a.ndim == 1 else a.shape[0]
    inter = np.ascontiguousarray(a if a.ndim == 1 else a.T)                                  # [frames][channels], as a file holds them
    return _Entry(inter.reshape(-1).view(np.uint8), None, array_sr, ch, 64 if a.dtype == np.float64 else 0, a.shape[-1])


def _crop_start(length: int, target: int, selection: str) -> int:
    """Where ``pad_or_window`` starts its window when it crops (audio_utils.py:52-62); ``random`` draws from torch's global CPU generator."""
    if selection == "random":
        return int(torch.randint(0, length - target + 1, ()).item())
    if selection == "center":
        return (length - target) // 2
    return 0


def plan_windows(lengths: Sequence[int], target_len: Optional[int] = None, window_selection: str = "start", dataset_max_len: Optional[int] = None,
                 starts: Optional[Sequence[int]] = None) -> Tuple[List[int], List[int], int]:
    """``(starts, valid lengths, T)`` of a batch whose clips hold ``lengths`` samples at the target rate.  Item by item, as the
    reference's Collater walks its batch: a clip longer than ``dataset_max_len`` is cropped to it first, then cropped or padded to
    ``target_len`` (``None``: the longest clip after the first step); a random start is drawn only by a step that crops, the dataset
    step first.  ``starts`` replaces the choice (the window then begins there and ends where the clip or a limit ends)."""
    if window_selection not in WINDOW_SELECTIONS:
        raise ValueError(f"Unknown window selection: {window_selection!r} (one of {WINDOW_SELECTIONS})")
    if len(lengths) == 0:
        raise ValueError("empty batch")
    if target_len is not None and target_len <= 0 or dataset_max_len is not None and dataset_max_len <= 0:
        raise ValueError(f"target_len={target_len}, dataset_max_len={dataset_max_len}: positive lengths expected")
    if starts is not None and len(starts) != len(lengths):
        raise ValueError(f"{len(starts)} starts for {len(lengths)} items")
    limit = [int(n) if dataset_max_len is None else min(int(n), int(dataset_max_len)) for n in lengths]
    T = int(target_len) if target_len is not None else max(limit)
    out_s, out_v = [], []
    for i, n in enumerate(lengths):
        n = int(n)
        if starts is not None:
            s0 = int(starts[i])
            if not 0 <= s0 < n:
                raise ValueError(f"item {i}: start {s0} outside its {n} samples")
            out_s.append(s0)
            out_v.append(min(T, limit[i], n - s0))
            continue
        s0 = _crop_start(n, limit[i], window_selection) if n > limit[i] else 0
        if limit[i] > T:
            s0 += _crop_start(limit[i], T, window_selection)
        out_s.append(s0)
        out_v.append(min(limit[i], T))
    return out_s, out_v, T


def pack_batch(entries: Sequence[_Entry], starts: Sequence[int], valids: Sequence[int], plan_index: Sequence[int]) -> Tuple[np.ndarray, int, int]:
    """``(descriptors, bytes to copy, bytes in all)`` of the packed buffer: the descriptors at its head, then every host payload, each at
    an 8-byte aligned offset -- that much is copied -- then the space the FLAC streams are decoded into on the device."""
    items = np.zeros(len(entries), dtype=ITEM_DTYPE)
    pos = (items.nbytes + 7) & ~7
    for flac_pass in (False, True):
        if flac_pass:
            copy_bytes = pos
        for i, e in enumerate(entries):
            if (e.flac is not None) != flac_pass:
                continue
            items[i] = (pos, e.frames, starts[i], valids[i], e.fmt, e.channels, plan_index[i])
            pos = (pos + e.nbytes + 7) & ~7
    return items, copy_bytes, pos


_BATCH_RESAMPLERS: Dict[Tuple[int, int, Optional[str]], Resampler] = {}
_BATCH_BUFFERS: Dict[int, Dict[str, Any]] = {}


def _grown(bufs: Dict[str, Any], name: str, nbytes: int, **kw) -> torch.Tensor:
    t = bufs.get(name)
    if t is None or t.numel() < nbytes:
        t = bufs[name] = torch.empty((max(nbytes, 1) * 5 // 4 + 255) & ~255, dtype=torch.uint8, **kw)
    return t


def _ingest(entries: Sequence[_Entry], target_sr: int, target_len: Optional[int], window_selection: str, starts, dataset_max_len: Optional[int],
            res_type: Optional[str], device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    import ctypes as C
    if window_selection not in WINDOW_SELECTIONS:
        raise ValueError(f"Unknown window selection: {window_selection!r} (one of {WINDOW_SELECTIONS})")
    if len(entries) == 0:
        raise ValueError("empty batch")
    _capi.require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        plans: List[Resampler] = []
        plan_index, lengths = [], []
        for e in entries:
            if e.sr == int(target_sr):
                plan_index.append(-1); lengths.append(e.frames)
                continue
            key = (e.sr, int(target_sr), res_type)
            if key not in _BATCH_RESAMPLERS:
                _BATCH_RESAMPLERS[key] = Resampler(e.sr, int(target_sr), res_type=res_type)
            rs = _BATCH_RESAMPLERS[key]
            if rs not in plans:
                plans.append(rs)
            plan_index.append(plans.index(rs)); lengths.append(rs.out_length(e.frames))
        win_s, win_v, T = plan_windows(lengths, target_len, window_selection, dataset_max_len, starts)
        items, copy_bytes, total_bytes = pack_batch(entries, win_s, win_v, plan_index)
        B = len(entries)
        handles = (C.c_void_p * max(len(plans), 1))(*[p._h for p in plans])
        ws_bytes = int(lib().avexhip_ingest_batch_workspace_bytes(items.ctypes.data, B, handles, len(plans), T))
        if ws_bytes == 0:
            raise ValueError(f"ingest_batch: {_capi.last_error()}")
        bufs = _BATCH_BUFFERS.setdefault(dev.index, {})
        if "copied" in bufs:
            bufs["copied"].synchronize()                  # the last batch's copy still reads the staging buffer
        host = _grown(bufs, "host", copy_bytes, pin_memory=True)
        raw = _grown(bufs, "raw", total_bytes, device=dev)
        ws = _grown(bufs, "ws", ws_bytes, device=dev)
        hv = host.numpy()
        hv[:items.nbytes] = items.view(np.uint8).reshape(-1)
        for i, e in enumerate(entries):
            if e.flac is None:
                off = int(items["offset"][i])
                hv[off:off + e.nbytes] = e.payload[:e.nbytes]
        stream = torch.cuda.current_stream().cuda_stream
        raw[:copy_bytes].copy_(host[:copy_bytes], non_blocking=True)
        bufs.setdefault("copied", torch.cuda.Event()).record()
        for i, e in enumerate(entries):
            if e.flac is not None:
                check(lib().avexhip_flac_decode_i32(e.flac._h, raw.data_ptr() + int(items["offset"][i]), 1, stream), "flac_decode_i32")
                e.flac.close()
        wav = torch.empty((B, T), dtype=torch.float32, device=dev)
        mask = torch.empty((B, T), dtype=torch.bool, device=dev)
        check(lib().avexhip_ingest_batch(raw.data_ptr(), total_bytes, items.ctypes.data, raw.data_ptr(), B, handles, len(plans), T, wav.data_ptr(), T,
                                         mask.data_ptr(), ws.data_ptr(), ws.numel(), stream), "ingest_batch")
    return wav, mask, torch.tensor(win_v, dtype=torch.int64)


def load_batch(sources: Sequence[Any], target_sr: int = 16000, target_len: Optional[int] = None, window_selection: str = "start",
               starts: Optional[Sequence[int]] = None, dataset_max_len: Optional[int] = None, res_type: Optional[str] = None,
               device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Files -> ``(wav [B, T] float32, padding_mask [B, T] bool (True = padding), lengths [B] int64)``; wav and mask on the device, the
    lengths (kept samples per row) on the host, where the windows are chosen.  ``sources`` mixes paths and bytes (WAV or FLAC) with
    ``(T,)`` / ``(C, T)`` float arrays or tensors taken to be at ``target_sr``.  Each row is the window ``[start, start + T)`` of the
    clip's mono resampling -- the bits :func:`load_audio` followed by a slice gives -- zero-padded behind its end; a float clip that
    holds a NaN or an Inf becomes a zero row.  ``target_len=None`` pads to the longest item; ``dataset_max_len`` crops longer clips
    first; windows are chosen by ``window_selection`` (``random`` | ``center`` | ``start``) or given in ``starts``; ``res_type`` as
    :class:`Resampler` takes it.  One host-to-device copy, a memset and two launches per batch (plus one decode per FLAC stream); the
staging, packed and workspace buffers are kept between calls and ordered by the current stream, so call it from one stream per device."""
    if len(sources) == 0:
        raise ValueError("empty batch")
    return _ingest([_open_source(s, int(target_sr)) for s in sources], target_sr, target_len, window_selection, starts, dataset_max_len, res_type, device)


def collate_labels(labels: Sequence[Any], num_labels: int) -> torch.Tensor:
    """The label tensor of the reference's Collater (dataset.py:341-373): all-int labels -> one-hot rows, or a ``[B, 1]`` zero tensor
    when ``num_labels == 0``; otherwise lists of class indices -> multi-hot rows, indices >= num_labels dropped."""
    if all(isinstance(lbl, (int, np.integer)) for lbl in labels):
        if num_labels > 0:
            return torch.nn.functional.one_hot(torch.tensor([int(v) for v in labels], dtype=torch.long), num_classes=num_labels).float()
        return torch.zeros((len(labels), 1), dtype=torch.float32)
    rows = []
    for lbl in labels:
        if num_labels <= 0:
            rows.append(torch.zeros(1, dtype=torch.float32))
            continue
        row = torch.zeros(num_labels, dtype=torch.float32)
        idx = lbl.clone().detach().long() if isinstance(lbl, torch.Tensor) else torch.tensor(lbl, dtype=torch.long)
        idx = idx[idx < num_labels]
        if len(idx) > 0:
            row[idx] = 1.0
        rows.append(row)
    return torch.stack(rows)


class Collater:
    """The reference's ``Collater`` (dataset.py:256-399) with the audio built on the device: ``__call__(batch)`` returns ``raw_wav``
    ``[B, T]`` float32 and ``padding_mask`` ``[B, T]`` bool (True = padding) on ``device``, ``label`` (host, as the reference) and
    ``text_label``.  An item's ``"audio"`` / ``"raw_wav"`` is an array at ``sr`` as in the reference, or a path / bytes of a WAV or
    FLAC file, resampled to ``sr``.  Window starts are drawn on the host exactly as the reference draws them, so under
    ``torch.manual_seed`` the windows are the reference's.  It touches the GPU: use it in the main process (``num_workers=0``).
    Deviation: a file is tested for NaN / Inf as decoded, before resampling; for arrays given at ``sr`` that is the reference's test."""

    def __init__(self, audio_max_length_seconds: int, sr: int, window_selection: str = "random", preprocessor: Optional[str] = None,
                 device: str = "cuda", batch_aug_processor: Any = None, num_labels: int = 0,
                 dataset_audio_max_length_seconds: Optional[int] = None) -> None:
        if batch_aug_processor is not None:
            raise NotImplementedError("batch_aug_processor (mixup) is a training-time augmentation; this Collater builds inference batches")
        if window_selection not in WINDOW_SELECTIONS:
            raise ValueError(f"Unknown window selection: {window_selection!r} (one of {WINDOW_SELECTIONS})")
        self.audio_max_length_seconds = audio_max_length_seconds
        self.dataset_audio_max_length_seconds = dataset_audio_max_length_seconds
        self.window_selection = window_selection
        self.preprocessor = preprocessor
        self.sr = sr
        self.device = device
        self.batch_aug_processor = None
        self.num_labels = num_labels

    def windows(self, lengths: Sequence[int]) -> Tuple[List[int], List[int], int]:
        """``plan_windows`` with this collater's limits (host only)."""
        limit = None if self.dataset_audio_max_length_seconds is None else self.dataset_audio_max_length_seconds * self.sr
        return plan_windows(lengths, self.audio_max_length_seconds * self.sr, self.window_selection, limit)

    def __call__(self, batch: Sequence[Dict[str, Any]]) -> Dict[str, Any]:
        if len(batch) == 0:
            raise ValueError("empty batch")
        entries, labels, text_labels = [], [], []
        for item in batch:
            entries.append(_open_source(item["audio" if "audio" in item else "raw_wav"], int(self.sr)))
            labels.append(item["label"] if "label" in item else 0)
            if "text_label" in item:
                txt = item["text_label"]
                if isinstance(txt, list) and len(txt) > 0:
                    txt = random.choice(txt)
                text_labels.append(txt)
        limit = None if self.dataset_audio_max_length_seconds is None else self.dataset_audio_max_length_seconds * self.sr
        wav, mask, _ = _ingest(entries, int(self.sr), self.audio_max_length_seconds * self.sr, self.window_selection, None, limit, None, self.device)
        return {"raw_wav": wav, "padding_mask": mask, "label": collate_labels(labels, self.num_labels), "text_label": text_labels}
