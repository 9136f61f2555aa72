"""Reader of tests/golden/collater.npz (written by tests/golden/make_collater_goldens.py from the reference's own Collater), shared by
the CPU and the GPU tests of the batched ingest."""
import json
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collater.npz")
_cache = {}


def cases():
    """name -> dict(kwargs, seed, items (as the reference's Collater took them), raw_wav, padding_mask, label); loaded once."""
    if not _cache:
        z = np.load(_PATH)
        meta = json.loads(bytes(z["meta"]).decode())
        for name, m in meta.items():
            items = []
            for i in range(m["n"]):
                it = {m["keys"][i]: z[f"{name}.in{i}"]}
                if m["labels"][i] is not None:
                    it["label"] = m["labels"][i]
                items.append(it)
            raw = z[f"{name}.raw_wav"]
            mask = np.unpackbits(z[f"{name}.padding_mask"], axis=1)[:, :raw.shape[1]].astype(bool)
            _cache[name] = dict(kwargs=m["kwargs"], seed=m["seed"], items=items, raw_wav=raw, padding_mask=mask, label=z[f"{name}.label"])
    return _cache


def audio(item):
    return item["audio"] if "audio" in item else item["raw_wav"]
