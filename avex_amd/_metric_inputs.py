"""Input handling shared by the device metrics (``retrieval.py``, ``clustering.py``): arrays or tensors, host or device, in; torch
tensors and dense class ids where the kernels want them out."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch


def _len0(x) -> int:
    return int(x.shape[0]) if isinstance(x, torch.Tensor) else int(np.asarray(x).shape[0])


def _as_tensor(x) -> torch.Tensor:
    """A torch tensor over a numeric `x` where it lives."""
    if isinstance(x, torch.Tensor):
        return x
    a = np.asarray(x)
    if a.dtype.kind not in "biuf":
        raise ValueError(f"dtype {a.dtype} is not numeric")
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.astype(np.int64)
    if a.dtype == np.float16:
        a = a.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a))


def _device_of(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _joint_ids(q: torch.Tensor, d: Optional[torch.Tensor], dev: torch.device):
    """Dense int32 class ids with `==` preserved across both sets."""
    if d is None:
        inv = torch.unique(q.to(dev), return_inverse=True)[1]
        ids = inv.to(torch.int32).contiguous()
        return ids, ids
    dt = torch.promote_types(q.dtype, d.dtype)
    inv = torch.unique(torch.cat([q.to(dev).to(dt), d.to(dev).to(dt)]), return_inverse=True)[1].to(torch.int32)
    return inv[: q.shape[0]].contiguous(), inv[q.shape[0]:].contiguous()


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)
