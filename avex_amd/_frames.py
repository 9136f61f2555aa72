"""The 512-sample frames of resident recordings on the host, for activity.py and soundscape.py (device side: ``csrc/rec_frames.h``)."""
from __future__ import annotations

import functools
from typing import Any, Tuple

import numpy as np
import torch

N_FFT = 512
N_BINS = N_FFT // 2 + 1


def _number(x: Any, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(float(x)):
        raise ValueError(f"{what}={x!r}: a finite number expected")
    return float(x)


def frame_count(n_samples: int, hop: int) -> int:
    return 0 if n_samples < N_FFT else (int(n_samples) - N_FFT) // int(hop) + 1


def tables() -> np.ndarray:
    """float32 ``[1536]``: the periodic Hann window, then the pairs ``(cos, -sin)(2 pi k / 512)``, computed in float64 and rounded."""
    a = 2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT
    return np.concatenate([0.5 - 0.5 * np.cos(a), np.stack([np.cos(a), -np.sin(a)], axis=1).reshape(-1)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _tables_on(dev: torch.device) -> torch.Tensor:
    return torch.from_numpy(tables()).to(dev)      # once per device, a blocking copy: every stream that comes later finds the table there


def _to_device(a: np.ndarray, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """A host array -> (its pinned copy, the device copy in flight); the caller keeps the pinned one until the stream has passed."""
    pinned = torch.from_numpy(a.view(np.uint8).reshape(-1)).pin_memory()
    return pinned, pinned.to(dev, non_blocking=True)


def recording_table(ws: Any, dtype: np.dtype, hop: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(table, int64 frame counts)`` of the recordings behind ``ws``; the caller adds to ``base``, ``n_samples`` and ``first_frame``."""
    first = np.asarray([w0 for w0, _ in ws.ranges], dtype=np.int64)
    rec = np.zeros(len(first), dtype=dtype)
    rec["base"], rec["n_samples"] = ws._table["base"][first], ws._table["n_samples"][first]
    frames = np.asarray([frame_count(int(n), hop) for n in rec["n_samples"]], dtype=np.int64)
    rec["first_frame"] = np.cumsum(frames) - frames
    return rec, frames
