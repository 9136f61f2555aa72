"""Golden generator for the batched ingest: the reference's own ``Collater`` (avex/data/dataset.py:256-399) run on small batches, written
to tests/golden/collater.npz.

``avex.data.dataset`` cannot be imported where these goldens are made (its ``esp_data`` dependency is absent), so the ``Collater`` class
node is taken out of the reference's dataset.py with ``ast`` at generation time and executed in a namespace that holds the real
``avex.data.audio_utils.pad_or_window`` (imported through tests/golden/_ref_import.py).  Nothing of the class is written anywhere.

Run where the reference is present; nothing under tests/ imports this module.  Only inputs, seeds and the reference's outputs are
stored.  Sample rates of 100 .. 1000 Hz keep the file small; one and two channels only, so that the channel mean is a single rounding
and the device result can be compared exactly.
"""
import ast
import json
import logging
import os
import random
import sys
from typing import Any, Optional

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF, import_reference  # noqa: E402


def reference_collater():
    import_reference()
    from avex.data.audio_utils import pad_or_window
    src = open(os.path.join(REF, "avex", "data", "dataset.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "Collater")
    ns = {"pad_or_window": pad_or_window, "torch": torch, "np": np, "random": random, "Any": Any, "Optional": Optional,
          "AugmentationProcessor": object, "logger": logging.getLogger("collater-goldens")}
    exec(compile(ast.Module(body=[node], type_ignores=[]), "<reference Collater>", "exec"), ns)
    return ns["Collater"]


def clip(rng, n, channels=1):
    a = (rng.standard_normal((channels, n)) * 0.3).astype(np.float32)
    return a[0] if channels == 1 else a


def batches():
    """name -> (constructor kwargs, seed, list of items).  Target 2 s, dataset limit 5 s where given."""
    rng = np.random.default_rng(20240611)
    out = {}
    for sel in ("random", "center", "start"):
        for limit in (None, 5):
            sr = {"random": 100, "center": 160, "start": 250}[sel]
            tgt = 2 * sr
            lens = [1, tgt - 37, tgt, tgt + 1, 3 * sr + 11, 5 * sr, 5 * sr + 1, 8 * sr + 3, 7 * sr]
            items = [{"audio": clip(rng, n), "label": i % 5} for i, n in enumerate(lens)]
            items.append({"audio": clip(rng, 6 * sr + 5, 2), "label": 2})                    # (2, T), longer than both limits
            items.append({"raw_wav": clip(rng, tgt - 10, 2), "label": 4})                    # (2, T), padded; the fallback key
            nan = clip(rng, 3 * sr); nan[sr + 3] = np.nan
            inf = clip(rng, tgt - 50, 2); inf[1, 7] = -np.inf
            items += [{"audio": nan, "label": 1}, {"audio": inf, "label": 3}]
            out[f"{sel}_{'limit' if limit else 'nolimit'}"] = (
                dict(audio_max_length_seconds=2, sr=sr, window_selection=sel, num_labels=5, dataset_audio_max_length_seconds=limit), 1000 + len(out), items)
    sr = 1000
    items = [{"audio": clip(rng, n), "label": i} for i, n in enumerate((700, 1000, 1300))]
    out["int_labels_no_classes"] = (dict(audio_max_length_seconds=1, sr=sr, window_selection="random", num_labels=0), 77, items)
    items = [{"audio": clip(rng, n), "label": lbl} for n, lbl in ((900, [0, 3]), (1000, [6]), (1500, [2, 9, 4]), (1200, []), (40, [5, 5, 1]))]
    out["index_lists"] = (dict(audio_max_length_seconds=1, sr=sr, window_selection="random", num_labels=6, dataset_audio_max_length_seconds=1), 78, items)
    items = [{"audio": clip(rng, n)} for n in (300, 2100)] + [{"audio": clip(rng, 1200), "label": [1]}]
    out["missing_labels"] = (dict(audio_max_length_seconds=1, sr=sr, window_selection="center", num_labels=0), 79, items)
    return out


def main():
    Collater = reference_collater()
    arrays, meta = {}, {}
    for name, (kw, seed, items) in batches().items():
        torch.manual_seed(seed)
        got = Collater(**kw)(items)
        assert got["raw_wav"].dtype == torch.float32 and got["padding_mask"].dtype == torch.bool
        meta[name] = {"kwargs": kw, "seed": seed, "n": len(items), "keys": ["audio" if "audio" in it else "raw_wav" for it in items],
                      "labels": [it.get("label") for it in items]}
        for i, it in enumerate(items):
            arrays[f"{name}.in{i}"] = it["audio" if "audio" in it else "raw_wav"]
        arrays[f"{name}.raw_wav"] = got["raw_wav"].numpy()
        arrays[f"{name}.padding_mask"] = np.packbits(got["padding_mask"].numpy(), axis=1)
        arrays[f"{name}.label"] = got["label"].numpy()
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "collater.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(meta)} batches")


if __name__ == "__main__":
    main()
