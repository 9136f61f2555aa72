#!/usr/bin/env python3
"""The LSTM recurrence kernel at a forced number of clips per workgroup.  lstm.hip reads AVEX_AMD_LSTM_LR once per process, so every tiling
needs a process of its own: test_gpu_probe_kernels.py starts this script three times, with AVEX_AMD_LSTM_LR = 1, 2, 4 in the child's
environment.
    AVEX_AMD_LSTM_LR=4 python tests/tools/lstm_forced_lr.py OUT.npz
For each (B, H) of _probe_ref.LSTM_FORCED_CASES (seeded inputs, T = LSTM_T) it runs lstm_layer forward and reverse and lstm_layer_pair into
buffers of B + LSTM_GUARD_CLIPS clips filled with NaN, of which the kernel is given the first B, and writes the whole buffers to OUT.npz
(``single_<B>_<H>``, ``pair_<B>_<H>``, and ``lr``).  It asserts nothing about the values: the parent does."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import _probe_ref as R
from avex_amd import kernels as K


def main():
    lr = int(os.environ["AVEX_AMD_LSTM_LR"])
    assert lr in (1, 2, 4), lr
    res = {"lr": np.int64(lr)}
    T, G = R.LSTM_T, R.LSTM_GUARD_CLIPS
    for B, H in R.LSTM_FORCED_CASES:
        xg, w, xgr, wr = [torch.from_numpy(a).cuda() for a in R.lstm_inputs(B, T, H)]
        single = torch.full((B + G, T, 2 * H), float("nan"), dtype=torch.float32, device="cuda")
        K.lstm_layer(xg, w, single[:B], col=0, reverse=False)
        K.lstm_layer(xgr, wr, single[:B], col=H, reverse=True)
        pair = torch.full((B + G, T, 2 * H), float("nan"), dtype=torch.float32, device="cuda")
        K.lstm_layer_pair(xg, w, xgr, wr, pair[:B])
        torch.cuda.synchronize()
        res[f"single_{B}_{H}"] = single.cpu().numpy()
        res[f"pair_{B}_{H}"] = pair.cpu().numpy()
    np.savez(sys.argv[1], **res)
    print(f"lstm_forced_lr: LR={lr}, {len(R.LSTM_FORCED_CASES)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
