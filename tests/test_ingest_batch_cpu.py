"""Batched ingest, host side (no GPU): the window arithmetic and the labels of ingest.Collater against the reference's own Collater
(tests/golden/collater.npz), the packed-buffer layout, the ABI number, the argument refusals."""
import numpy as np
import pytest
import torch

import _collater_golden as G
from avex_amd import _capi, ingest


def _mono(a):
    """The reference's channel mean for one or two channels: a single rounding."""
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 1:
        return a
    assert a.shape[0] == 2
    return (a[0] + a[1]) / np.float32(2)


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_windows_and_labels_reproduce_the_reference_collater(name):
    """Under the recorded seed, the starts and valid lengths the host chooses cut exactly the reference's rows out of the inputs (so the
    draws come in the reference's order: per item, the dataset-limit crop before the model-length crop, and only when a step crops),
    the mask is the reference's, and the label tensor is the reference's."""
    c = G.cases()[name]
    col = ingest.Collater(**c["kwargs"])
    clips = [G.audio(it) for it in c["items"]]
    torch.manual_seed(c["seed"])
    starts, valids, T = col.windows([a.shape[-1] for a in clips])
    assert T == c["raw_wav"].shape[1] == c["kwargs"]["audio_max_length_seconds"] * c["kwargs"]["sr"]
    for b, a in enumerate(clips):
        assert 0 <= starts[b] and 0 < valids[b] <= T and starts[b] + valids[b] <= a.shape[-1]
        row = np.zeros(T, np.float32)
        if np.isfinite(a).all():
            row[:valids[b]] = _mono(a)[starts[b]:starts[b] + valids[b]]
        assert np.array_equal(row, c["raw_wav"][b]), (name, b)
        assert np.array_equal(np.arange(T) >= valids[b], c["padding_mask"][b]), (name, b)
    labels = [it["label"] if "label" in it else 0 for it in c["items"]]
    got = ingest.collate_labels(labels, c["kwargs"]["num_labels"])
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), c["label"])


def test_window_arithmetic_edges():
    s, v, T = ingest.plan_windows([5, 9, 7], None, "center")
    assert (s, v, T) == ([0, 0, 0], [5, 9, 7], 9)                       # target_len=None: the longest item, nothing cropped
    s, v, T = ingest.plan_windows([5, 9, 7], None, "center", dataset_max_len=6)
    assert (s, v, T) == ([0, 1, 0], [5, 6, 6], 6)
    s, v, T = ingest.plan_windows([10, 3, 100], 4, "start", starts=[6, 1, 96])
    assert (s, v, T) == ([6, 1, 96], [4, 2, 4], 4)
    s, v, T = ingest.plan_windows([10, 100], 8, "start", dataset_max_len=5, starts=[7, 50])
    assert (s, v, T) == ([7, 50], [3, 5], 8)
    state = torch.get_rng_state()
    ingest.plan_windows([4, 8, 8], 8, "random")                         # nothing crops: nothing is drawn
    assert torch.equal(state, torch.get_rng_state())
    torch.manual_seed(5)
    want = [int(torch.randint(0, 20 - 10 + 1, ()).item()) + int(torch.randint(0, 10 - 8 + 1, ()).item()), int(torch.randint(0, 9 - 8 + 1, ()).item())]
    torch.manual_seed(5)
    assert ingest.plan_windows([20, 9], 8, "random", dataset_max_len=10)[0] == want
    for bad in ([10], [10, 10, 10]):
        with pytest.raises(ValueError):
            ingest.plan_windows([10, 10], 4, "start", starts=bad)
    with pytest.raises(ValueError):
        ingest.plan_windows([10], 4, "start", starts=[10])


def test_descriptor_packing():
    rng = np.random.default_rng(3)
    srcs = [rng.standard_normal(13).astype(np.float32),                  # 52 bytes: the next offset has to be rounded up
            rng.standard_normal((3, 7)),                                 # float64, three channels
            rng.standard_normal((2, 5)).astype(np.float32),
            torch.zeros(9)]
    entries = [ingest._open_source(s, 16000) for s in srcs]
    assert [(e.fmt, e.channels, e.frames, e.nbytes) for e in entries] == [(0, 1, 13, 52), (64, 3, 7, 168), (0, 2, 5, 40), (0, 1, 9, 36)]
    assert np.array_equal(entries[2].payload.view(np.float32).reshape(5, 2), srcs[2].T)      # interleaved [frames][channels]
    entries[1].flac = object()                                           # stands for a FLAC stream: space behind the copied part
    items, copy_bytes, total = ingest.pack_batch(entries, [0, 1, 2, 3], [13, 6, 3, 6], [-1, 0, -1, 1])
    assert items.dtype.itemsize == 40 and items.dtype == ingest.ITEM_DTYPE
    assert items["offset"].tolist() == [160, 296, 216, 256] and copy_bytes == 296 and total == 464
    spans = [(int(o), int(o) + e.nbytes) for o, e in zip(items["offset"], entries)]
    assert all(lo % 8 == 0 and lo >= items.nbytes and hi <= total for lo, hi in spans)
    assert all(a[1] <= b[0] for a, b in zip(sorted(spans), sorted(spans)[1:]))      # disjoint
    assert all((lo >= copy_bytes) if i == 1 else (hi <= copy_bytes) for i, (lo, hi) in enumerate(spans))
    assert items["plan"].tolist() == [-1, 0, -1, 1] and items["start"].tolist() == [0, 1, 2, 3] and items["valid"].tolist() == [13, 6, 3, 6]
    assert items["sample_format"].tolist() == [0, 64, 0, 0] and items["channels"].tolist() == [1, 3, 2, 1] and items["frames"].tolist() == [13, 7, 5, 9]


def test_header_abi_is_13_and_declares_the_batch_entry_points():
    assert _capi.header_abi_version() >= 13
    for name in ("avexhip_ingest_batch", "avexhip_ingest_batch_workspace_bytes"):
        assert name in _capi.SYMBOLS


def test_argument_refusals():
    with pytest.raises(NotImplementedError):
        ingest.Collater(1, 100, batch_aug_processor=object())
    with pytest.raises(ValueError, match="window selection"):
        ingest.Collater(1, 100, window_selection="end")
    with pytest.raises(ValueError, match="window selection"):
        ingest.plan_windows([10], 4, "end")
    with pytest.raises(ValueError, match="window selection"):
        ingest.load_batch([np.zeros(8, np.float32)], window_selection="end")
    with pytest.raises(ValueError, match="empty"):
        ingest.load_batch([])
    with pytest.raises(ValueError, match="empty"):
        ingest.Collater(1, 100)([])
    with pytest.raises(ValueError):
        ingest.load_batch([b"OggS" + bytes(64)])                         # a container that is not decoded here
    with pytest.raises(ValueError):
        ingest.load_batch([np.zeros((2, 3, 4), np.float32)])


def test_c_entry_refuses_on_the_host(built_lib):
    """avexhip_ingest_batch checks its descriptors on the host and returns before it touches a device: these calls run without one (the
    "device" pointers are host arrays that a refused call never reads)."""
    lib = built_lib
    fake = np.zeros(4096, dtype=np.uint8)
    out = np.full(2 * 64, 7.0, dtype=np.float32)
    msk = np.full(2 * 64, 7, dtype=np.uint8)

    def items(**over):
        it = np.zeros(2, dtype=ingest.ITEM_DTYPE)
        it[0] = (128, 100, 0, 64, 16, 1, -1)
        it[1] = (512, 64, 0, 64, 0, 2, -1)
        for k, v in over.items():
            it[k][0] = v
        return it

    def call(it, B=2, T_out=64, raw_bytes=4096, ws_bytes=1 << 20):
        rc = lib.avexhip_ingest_batch(fake.ctypes.data, raw_bytes, it.ctypes.data, fake.ctypes.data, B, None, 0, T_out, out.ctypes.data, 64, msk.ctypes.data,
                                      fake.ctypes.data, ws_bytes, None)
        return rc, _capi.last_error()

    need = lib.avexhip_ingest_batch_workspace_bytes(items().ctypes.data, 2, None, 0, 64)
    assert need == 256 + 2 * 64 * 4                                      # the flags, then the longest span per item
    for rc, msg in (call(items(valid=65)), call(items(start=37)), call(items(start=-1)), call(items(offset=4096 - 192)),
                    call(items(offset=-8)), call(items(offset=132)), call(items(), raw_bytes=1000), call(items(plan=0)), call(items(plan=-2)),
                    call(items(sample_format=12)), call(items(channels=65)), call(items(frames=0)), call(items(), B=0),
                    call(np.zeros(65536, dtype=ingest.ITEM_DTYPE), B=65536), call(items(), T_out=0)):
        assert rc == -1 and msg.startswith("ingest_batch"), (rc, msg)
    rc, msg = call(items(), ws_bytes=need - 1)
    assert rc == -4 and "workspace" in msg
    assert lib.avexhip_ingest_batch_workspace_bytes(items(valid=65).ctypes.data, 2, None, 0, 64) == 0
    assert (out == 7.0).all() and (msk == 7).all()
