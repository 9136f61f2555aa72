"""avex_amd.examples without a GPU: the NumPy restatement against hand-written cases, the ABI 17 bindings and struct layout, the
workspace size, the refusals of the entry points, the segment tables, and every ValueError of the Python layer."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _examples_ref as E
from avex_amd import _capi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMS = ("avexhip_examples_max_top_m", "avexhip_examples_workspace_bytes", "avexhip_examples_score", "avexhip_examples_class_mean")
F = np.float32


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_top_m_sum_runs_from_the_largest_down():
    # 2^24 + 1 + 1: from the largest down each 1 is lost to rounding (2^24 + 1 rounds to even, 2^24); the other way round 1 + 1 = 2 survives
    big = F(2.0 ** 24)
    v, near = E.class_value([1.0, big, 1.0], 3)
    assert v == F(big / F(3.0)) and near == 1
    assert F(F(F(1.0) + F(1.0)) + big) / F(3.0) != v                                           # the ascending sum is another number
    v, _ = E.class_value([0.5, 0.25, 1.0, 0.125], 2)
    assert v == F(0.75)                                                                         # (1.0 + 0.5) / 2: only the two largest
    v, _ = E.class_value([0.5, 0.25, 1.0, 0.125], 1)
    assert v == F(1.0)
    v, _ = E.class_value([1.0, 1.0, 0.25], 3)
    assert v == F(F(2.25) / F(3.0))                                                             # a correctly rounded fp32 division
    with pytest.raises(AssertionError):
        E.class_value([1.0], 17)


def test_fewer_rows_than_top_m_and_empty_classes():
    v, near = E.class_value([0.5, 0.25], 16)
    assert v == F(0.375) and near == 0                                                          # divided by the two kept, not by top_m
    v, near = E.class_value([], 4)
    assert np.isnan(v) and near == -1
    sim = np.array([[0.5, 0.25, 1.0]], dtype=F)
    s, near = E.score(sim, [0, 2, 2], 4, top_m=2)                                               # classes 1 and 3 are empty
    assert s.dtype == F and near.dtype == np.int32 and s.shape == (1, 4)
    assert s[0, 0] == F(0.5) and s[0, 2] == F(0.625) and np.isnan(s[0, 1]) and np.isnan(s[0, 3])
    assert near[0].tolist() == [0, -1, 2, -1]


def test_nan_is_skipped_and_minus_zero_is_zero():
    v, near = E.class_value([np.nan, 0.5, np.nan, 0.25], 3)
    assert v == F(0.375) and near == 1                                                          # two numbers: divided by two
    v, near = E.class_value([np.nan, np.nan], 1)
    assert np.isnan(v) and near == -1
    v, near = E.class_value([-0.0], 1)
    assert v == 0.0 and not np.signbit(v) and near == 0
    v, near = E.class_value([0.0, -0.0, -1.0], 2)                                               # -0.0 ties with +0.0: the earlier row is the nearest
    assert v == 0.0 and not np.signbit(v) and near == 0
    v, near = E.class_value([-0.0, 0.0], 1)
    assert near == 0 and not np.signbit(v)
    v, near = E.class_value([-np.inf, np.inf, 1.0], 1)                                          # infinities are numbers
    assert v == np.inf and near == 1
    s, near = E.score(np.array([[np.nan, np.nan, np.nan]], dtype=F), [0, 1, -1], 2, top_m=1, mode="margin")      # a NaN window
    assert np.isnan(s).all() and (near == -1).all()


def test_margin_and_nearest_ties():
    sim = np.array([[0.5, 1.0, 0.5, 1.0, 0.25, 0.75],
                    [0.1, 0.2, 0.3, 0.4, np.nan, np.nan]], dtype=F)
    labels = [1, 0, 0, 0, -1, -1]
    s, near = E.score(sim, labels, 2, top_m=2, mode="similarity")
    assert s[0].tolist() == [F(1.0), F(0.5)] and s[1].tolist() == [F(F(0.4) + F(0.3)) / F(2.0), F(0.1)]
    assert near.tolist() == [[1, 0], [3, 0]]                                                    # rows 1 and 3 tie at 1.0: the lower row
    m, near_m = E.score(sim, labels, 2, top_m=2, mode="margin")
    assert m[0].tolist() == [F(1.0) - F(0.5), F(0.5) - F(0.5)] and np.array_equal(near_m, near)
    assert np.isnan(m[1]).all() and near_m[1].tolist() == [3, 0]                                # no background number: NaN carries, nearest stays
    with pytest.raises(ValueError):
        E.score(sim, labels, 2, mode="ratio")
    # the vectorised form is the scalar one
    rng = np.random.RandomState(3)
    sim = rng.randint(-3, 4, size=(40, 30)).astype(F) / F(4.0)
    sim[rng.rand(40, 30) < 0.2] = np.nan
    sim[rng.rand(40, 30) < 0.1] = -0.0
    labels = rng.randint(-1, 5, size=30)
    for top_m in (1, 2, 5, 16):
        s, near = E.score(sim, labels, 6, top_m=top_m)
        for n in range(40):
            for c in range(6):
                cols = np.flatnonzero(labels == c)
                v, p = E.class_value(sim[n, cols], top_m)
                assert (np.isnan(v) and np.isnan(s[n, c])) or (v == s[n, c] and np.signbit(v) == np.signbit(s[n, c])), (top_m, n, c)
                assert near[n, c] == (cols[p] if p >= 0 else -1)


def test_prototypes_are_summed_sequentially():
    big = F(2.0 ** 24)
    rows = np.array([[big, 1.0], [1.0, 1.0], [1.0, 2.0], [7.0, 7.0], [1.0, 4.0]], dtype=F)
    means, lab = E.prototypes(rows, [0, 0, 0, -1, 2], 4)
    assert lab.tolist() == [0, 2, -1] and means.dtype == F                                      # classes 1 and 3 are empty; the background is last
    assert means[0].tolist() == [F(big / F(3.0)), F(F(4.0) / F(3.0))]                           # 2^24 + 1 + 1 in that order loses both ones
    assert means[1].tolist() == [1.0, 4.0] and means[2].tolist() == [7.0, 7.0]
    means, lab = E.prototypes(rows[[1, 2, 0]], [0, 0, 0], 1)                                    # another order of adding, another sum
    assert means[0, 0] == F(F(big + F(2.0)) / F(3.0))
    means, lab = E.prototypes(np.zeros((0, 3), dtype=F), [], 2)
    assert means.shape == (0, 3) and lab.shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ the bindings
def test_bindings(built_lib):
    assert _capi.header_abi_version() >= 17
    for name in SYMS:
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name
    hdr = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/avexhip.h").read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(avexhip_examples_[a-z0-9_]+)\s*\(", hdr))) == sorted(SYMS)
    assert built_lib.avexhip_examples_max_top_m() == 16 == examples.MAX_TOP_M == E.MAX_TOP_M


def test_examples_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of the ABI 17 struct as gcc sees include/avexhip.h == the ctypes mirror."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = {"avexhip_examples_args": _capi.ExamplesArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/avexhip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(out[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_workspace_is_monotone_and_knows_no_number_of_windows(built_lib):
    ws = built_lib.avexhip_examples_workspace_bytes
    assert len(_capi.SYMBOLS["avexhip_examples_workspace_bytes"][1]) == 4                                   # batch, n_segments, top_m, dpad: no N
    assert "n_windows" not in inspect.signature(examples.segment_tables).parameters
    base = (4096, 300, 5, 768)
    b0 = ws(*base)
    need = 8 * 4096 * 300 * 5 + 4 * 4096 * 768                                                              # the lists and the prepared queries
    assert need <= b0 <= need + 4 * 4096 + 3 * 256
    for axis, steps in enumerate(((1, 2, 127, 128, 4096, 65536), (1, 2, 79, 300, 10000), (1, 2, 5, 15, 16), (32, 64, 768, 4096))):
        sizes = []
        for v in steps:
            a = list(base)
            a[axis] = v
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (axis, sizes)
    for bad in ((0, 300, 5, 768), (4096, 0, 5, 768), (4096, 300, 0, 768), (4096, 300, 17, 768), (4096, 300, 5, 0), (4096, 300, 5, 40), (-1, 300, 5, 768)):
        assert ws(*bad) == 0, bad


def _args(**kw):
    fake = 1 << 20                                                        # a 16-byte aligned number: never dereferenced, the call is refused first
    a = _capi.ExamplesArgs()
    a.bank, a.row_id, a.m, a.d, a.n_classes, a.n_segments, a.batch = fake, fake, 300, 64, 4, 5, 8
    a.segments, a.tile_segments, a.class_segments = fake, fake, fake
    a.query, a.ld_query, a.n, a.top_m, a.mode, a.normalise = fake, 64, 4, 5, 0, 1
    a.workspace, a.workspace_bytes = fake, 1 << 30
    a.scores, a.ld_scores, a.nearest, a.ld_nearest = fake, 4, None, 0
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def test_entry_points_refuse_bad_shapes(built_lib):
    """rc -1 and a message that names the offending number, before the device is touched."""
    fake = 1 << 20
    lib = built_lib

    def refused(rc, *words):
        msg = _capi.last_error()
        assert rc == -1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    score = lib.avexhip_examples_score
    refused(score(None, None), "examples_score", "null")
    for name in ("bank", "row_id", "segments", "tile_segments", "class_segments", "query", "workspace", "scores"):
        refused(score(C.byref(_args(**{name: None})), None), "null")
    refused(score(C.byref(_args(m=0)), None), "m 0")
    refused(score(C.byref(_args(m=1 << 31)), None), str(1 << 31))
    refused(score(C.byref(_args(d=0)), None), "d 0")
    refused(score(C.byref(_args(n_classes=0)), None), "n_classes 0")
    refused(score(C.byref(_args(n_segments=2)), None), "n_segments 2")                                       # 300 rows are three tiles
    refused(score(C.byref(_args(n_segments=8)), None), "n_segments 8")                                       # at most tiles + classes
    refused(score(C.byref(_args(batch=0)), None), "batch 0")
    refused(score(C.byref(_args(n=0)), None), "n 0")
    refused(score(C.byref(_args(n=9)), None), "n 9")
    refused(score(C.byref(_args(top_m=0)), None), "top_m 0")
    refused(score(C.byref(_args(top_m=17)), None), "top_m 17")
    refused(score(C.byref(_args(mode=2)), None), "mode 2")
    refused(score(C.byref(_args(normalise=2)), None), "normalise 2")
    refused(score(C.byref(_args(ld_query=63)), None), "ld_query 63")
    refused(score(C.byref(_args(ld_scores=3)), None), "ld_scores 3")
    refused(score(C.byref(_args(nearest=fake, ld_nearest=3)), None), "ld_nearest 3")
    refused(score(C.byref(_args(stages=4)), None), "stages 4")
    rc = score(C.byref(_args(workspace_bytes=1000)), None)                                                   # a workspace too small has its own code
    assert rc == -4 and "1000 B" in _capi.last_error()
    mean = lib.avexhip_examples_class_mean
    refused(mean(None, 10, 64, fake, fake, 2, fake, 64, None), "examples_class_mean", "null")
    refused(mean(fake, 0, 64, fake, fake, 2, fake, 64, None), "n_rows 0")
    refused(mean(fake, 10, 0, fake, fake, 2, fake, 64, None), "d 0")
    refused(mean(fake, 10, 64, fake, fake, 0, fake, 64, None), "n_out 0")
    refused(mean(fake, 10, 64, fake, fake, 65536, fake, 64, None), "n_out 65536")
    refused(mean(fake, 10, 64, fake, fake, 2, fake, 63, None), "ld_out 63")


# ------------------------------------------------------------------------------------------------------------------ the segment tables
def _check_tables(counts):
    """The properties the kernels rely on, whatever the counts: segments tile the columns in order, stay inside one class and one tile,
    and both indexes find them."""
    counts = np.asarray(counts, dtype=np.int64)
    t = examples.segment_tables(counts)
    seg, tile_seg, class_seg = t["segments"], t["tile_segments"], t["class_segments"]
    assert seg.dtype == tile_seg.dtype == class_seg.dtype == np.int32 and seg.flags.c_contiguous and class_seg.flags.c_contiguous
    m = int(counts.sum())
    n_tiles = (m + 127) // 128
    assert seg.shape[1] == 4 and tile_seg.shape == (n_tiles + 1,) and class_seg.shape == (len(counts), 2)
    assert n_tiles <= len(seg) <= n_tiles + len(counts) - 1 or m == 0
    starts = np.cumsum(counts) - counts
    label_of = np.repeat(np.arange(len(counts)), counts)
    covered = np.concatenate([np.arange(a, b + 1) for _, a, b, _ in seg]) if len(seg) else np.zeros(0, dtype=np.int64)
    assert np.array_equal(covered, np.arange(m))                                                            # every column once, in order
    for s, (c, a, b, tl) in enumerate(seg):
        assert a <= b and a // 128 == b // 128 == tl and (label_of[a:b + 1] == c).all()
        assert tile_seg[tl] <= s < tile_seg[tl + 1] and class_seg[c, 0] <= s <= class_seg[c, 1]
    assert tile_seg[0] == 0 and tile_seg[-1] == len(seg) and (np.diff(tile_seg) >= 1).all()
    for c in range(len(counts)):
        if counts[c] == 0:
            assert class_seg[c].tolist() == [0, -1]
        else:
            s0, s1 = class_seg[c]
            assert (seg[s0:s1 + 1, 0] == c).all() and seg[s0, 1] == starts[c] and seg[s1, 2] == starts[c] + counts[c] - 1
            assert s1 - s0 == (starts[c] + counts[c] - 1) // 128 - starts[c] // 128
    return t


def test_segment_tables():
    t = _check_tables([128, 5, 0])                                                                          # a class ending exactly on a tile edge; no background
    assert t["segments"].tolist() == [[0, 0, 127, 0], [1, 128, 132, 1]] and t["tile_segments"].tolist() == [0, 1, 2]
    assert t["class_segments"].tolist() == [[0, 0], [1, 1], [0, -1]]
    t = _check_tables([100, 300, 7])                                                                        # a class spanning three tiles (plus a fourth's start)
    assert t["segments"].tolist() == [[0, 0, 99, 0], [1, 100, 127, 0], [1, 128, 255, 1], [1, 256, 383, 2], [1, 384, 399, 3], [2, 400, 406, 3]]
    assert t["class_segments"].tolist() == [[0, 0], [1, 4], [5, 5]] and t["tile_segments"].tolist() == [0, 2, 3, 4, 6]
    t = _check_tables([50, 257, 0])                                                                         # 78 + 128 + 51: exactly three tiles
    assert t["class_segments"][1].tolist() == [1, 3]
    t = _check_tables([1] * 128 + [0])                                                                      # 128 one-row classes in one tile
    assert len(t["segments"]) == 128 and t["tile_segments"].tolist() == [0, 128] and (t["segments"][:, 1] == t["segments"][:, 2]).all()
    t = _check_tables([1] * 128 + [3])                                                                      # ... and the background behind them
    assert t["segments"][-1].tolist() == [128, 128, 130, 1]
    t = _check_tables([0, 0, 130, 0, 0, 2, 0, 0, 9])                                                        # empty classes at the start, in the middle, at the end
    assert t["class_segments"].tolist() == [[0, -1], [0, -1], [0, 1], [0, -1], [0, -1], [2, 2], [0, -1], [0, -1], [3, 3]]
    t = _check_tables([0, 0, 130, 0, 0, 2, 0, 0, 0])                                                        # background absent
    assert t["class_segments"][-1].tolist() == [0, -1] and len(t["segments"]) == 3
    t = _check_tables([0, 0, 5])                                                                            # background only
    assert t["segments"].tolist() == [[2, 0, 4, 0]]
    _check_tables([1])
    rng = np.random.RandomState(7)
    for _ in range(20):
        _check_tables(rng.randint(0, 400, size=rng.randint(1, 12)) * (rng.rand() < 0.8))
    t = examples.segment_tables([0, 0])
    assert t["segments"].shape == (0, 4) and t["tile_segments"].tolist() == [0]
    for bad in ([], [3, -1]):
        with pytest.raises(ValueError):
            examples.segment_tables(bad)


# ------------------------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture()
def no_gpu(monkeypatch):
    """Whatever reaches the device fails the test: every ValueError below is raised before _capi.require_gpu()."""
    def boom():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_capi, "require_gpu", boom)


def _filled(dim=8, labels=(0, 1, 1, -1), **kw):
    """A bank that claims rows without having touched a device (scores are refused before they look at them)."""
    bank = examples.ExampleBank(dim, **kw)
    bank._labels = [np.asarray(labels, dtype=np.int64)]
    bank._n = len(labels)
    bank._max_label = int(max(labels))
    return bank


def test_constructor_errors(no_gpu):
    for bad in (dict(dim=0), dict(dim=-3), dict(dim=2.5), dict(dim=True), dict(dim=8, metric="euclidean"), dict(dim=8, metric=None), dict(dim=8, n_classes=0),
                dict(dim=8, n_classes=-1), dict(dim=8, n_classes=2.0), dict(dim=8, n_classes=2, class_names=["a"])):
        with pytest.raises(ValueError):
            examples.ExampleBank(**bad)
    bank = examples.ExampleBank(40, metric="dot", class_names=["gibbon", "owl"])
    assert len(bank) == 0 and bank.dpad == 64 and bank.metric == "dot" and bank.n_classes == 0 and bank.counts.tolist() == [0]
    assert examples.ExampleBank(8, n_classes=3).counts.tolist() == [0, 0, 0, 0]
    bank = _filled()
    assert bank.n_classes == 2 and bank.counts.tolist() == [1, 2, 1] and bank.labels.tolist() == [0, 1, 1, -1] and len(bank) == 4
    assert _filled(n_classes=5).counts.tolist() == [1, 2, 0, 0, 0, 1]


def test_add_errors(no_gpu):
    bank = examples.ExampleBank(8, n_classes=3)
    x = np.zeros((4, 8), dtype=np.float32)
    for bad in (np.zeros((4, 7), dtype=np.float32), np.zeros((8,), dtype=np.float32), torch.zeros(4, 8, 1), np.zeros((4, 9))):      # width mismatch
        with pytest.raises(ValueError):
            bank.add(bad, 0)
    for bad in ([0, 1, 2], [0, 1, 2, 3], [0, 1, 2, -2], 3, -2, [0.0, 1.0, 2.0, 0.0], [[0, 1, 2, 0]], [True, False, True, False], "owl"):      # label out of range
        with pytest.raises(ValueError):
            bank.add(x, bad)
    free = examples.ExampleBank(8)                                         # no n_classes: any class, but nothing under the background
    with pytest.raises(ValueError):
        free.add(x, [0, 1, -2, 5])
    assert bank.add(np.zeros((0, 8), dtype=np.float32), []) == range(0, 0) and len(bank) == 0
    assert bank.add(np.zeros((0, 8), dtype=np.float32), 2) == range(0, 0)
    big = _filled()
    big._n = (1 << 31) - 2
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        big.add(np.zeros((2, 8), dtype=np.float32), 0)
    with pytest.raises(ValueError):
        bank.add_clips(None, [np.zeros(16000, dtype=np.float32)], [0, 1])                                   # two labels for one clip
    with pytest.raises(ValueError):
        bank.add_clips(None, [np.zeros(16000, dtype=np.float32)], [3])


def test_score_errors(no_gpu):
    bank = _filled()
    q = np.zeros((3, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="empty"):
        examples.ExampleBank(8).score(q)
    with pytest.raises(ValueError, match="empty"):
        examples.ExampleBank(8).scorer()
    with pytest.raises(ValueError, match="empty"):
        examples.detect_events_by_example(None, examples.ExampleBank(8), ["a.wav"], 1.0, on=0.5)
    for bad_q in (np.zeros((3, 7), dtype=np.float32), np.zeros(8, dtype=np.float32), torch.zeros(3, 9)):
        with pytest.raises(ValueError):
            bank.score(bad_q)
    for kw in (dict(top_m=0), dict(top_m=17), dict(top_m=-1), dict(top_m=2.0), dict(top_m=True), dict(mode="ratio"), dict(mode=None), dict(mode="Margin"),
               dict(batch_size=0), dict(batch_size=-4), dict(batch_size=1.5)):
        with pytest.raises(ValueError):
            bank.score(q, **kw)
        with pytest.raises(ValueError):
            bank.scorer(**kw)
        if "batch_size" not in kw:
            with pytest.raises(ValueError):
                examples.detect_events_by_example(None, bank, ["a.wav"], 1.0, on=0.5, **kw)
    no_bg = _filled(labels=(0, 1, 1))
    with pytest.raises(ValueError, match="background"):
        no_bg.score(q, mode="margin")
    with pytest.raises(ValueError, match="background"):
        no_bg.scorer(mode="margin")
    with pytest.raises(ValueError, match="background"):
        examples.detect_events_by_example(None, no_bg, ["a.wav"], 1.0, on=0.5, mode="margin")
    only_bg = _filled(labels=(-1, -1))
    with pytest.raises(ValueError, match="no class"):
        only_bg.score(q)
    assert callable(bank.scorer(top_m=5, mode="margin"))


def test_state_dict_errors_and_signatures(no_gpu):
    empty = examples.ExampleBank(8, n_classes=3, metric="dot", class_names=["a", "b", "c"]).state_dict()    # an empty bank round-trips without a device
    assert empty["rows"].shape == (0, 8) and str(empty["metric"]) == "dot" and int(empty["n_classes"]) == 3
    back = examples.ExampleBank.from_state_dict(empty)
    assert len(back) == 0 and back.metric == "dot" and back.dim == 8 and back.n_classes == 3 and back.class_names == ["a", "b", "c"]
    free = examples.ExampleBank.from_state_dict(examples.ExampleBank(8).state_dict())
    assert free.n_classes == 0 and free.class_names is None and free._n_classes is None
    st = dict(empty, rows=np.zeros((3, 7), dtype=np.float32), labels=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError):
        examples.ExampleBank.from_state_dict(st)                           # rows narrower than dim
    st = dict(empty, rows=np.zeros((3, 8), dtype=np.float32), labels=np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError):
        examples.ExampleBank.from_state_dict(st)
    st = dict(empty, rows=np.zeros((3, 8), dtype=np.float32), labels=np.array([0, 1, 3], dtype=np.int32))
    with pytest.raises(ValueError):
        examples.ExampleBank.from_state_dict(st)                           # a label outside the classes
    with pytest.raises(ValueError):
        examples.ExampleBank.from_state_dict(dict(empty, metric=np.asarray("l2")))
    sig = inspect.signature(examples.ExampleBank.score)
    assert [p for p in sig.parameters][:2] == ["self", "embeddings"] and sig.parameters["top_m"].default == 1 and sig.parameters["mode"].default == "similarity"
    assert sig.parameters["batch_size"].default == 4096 and sig.parameters["return_nearest"].default is False
    assert sig.parameters["top_m"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(examples.ExampleBank.__init__)
    assert [p for p in sig.parameters] == ["self", "dim", "n_classes", "metric", "device", "class_names"] and sig.parameters["metric"].default == "cosine"
    sig = inspect.signature(examples.detect_events_by_example)
    assert [p for p in sig.parameters][:5] == ["model", "bank", "sources", "window_s", "hop_s"] and sig.parameters["top_m"].kind is inspect.Parameter.KEYWORD_ONLY
    import avex_amd
    assert avex_amd.ExampleBank is examples.ExampleBank and avex_amd.detect_events_by_example is examples.detect_events_by_example
    assert "ExampleBank" in avex_amd.__all__ and "detect_events_by_example" in avex_amd.__all__
