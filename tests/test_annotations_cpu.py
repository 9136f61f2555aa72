"""Annotations and detection scoring without a GPU: validation, hand-worked merges and cells, a Raven table, the matching walk against a
brute-force maximum matching (the claim the kernels rest on), compatibility at exact boundaries, the bindings and the argument checks of
the entry points, and the public names."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _annotations_ref as A
import avex_amd
from avex_amd import _capi, annotations
from avex_amd.annotations import Annotations, WindowPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IOUS = (1 / 16, 0.2, 0.3, 0.5, 0.75, 1.0)


def test_validation_refusals():
    ok = dict(recording=[0, 1], class_id=[0, 2], start_s=[0.0, 1.5], end_s=[1.0, 2.0])
    a = Annotations(**ok)
    assert a.n_classes == 3 and len(a) == 2 and a.class_names is None and a.start_s.dtype == np.float64 and a.recording.dtype == np.int64
    assert Annotations(**ok, n_classes=5).n_classes == 5 and Annotations(**ok, class_names=["a", "b", "c"]).class_names == ("a", "b", "c")
    assert Annotations([], [], [], []).n_classes == 1
    for kw in (dict(start_s=[0.0, float("nan")]), dict(end_s=[1.0, float("inf")]), dict(end_s=[1.0, 1.5]), dict(end_s=[1.0, 1.0]), dict(start_s=[-0.5, 1.5]),
               dict(recording=[0, -1]), dict(class_id=[-1, 2]), dict(n_classes=2), dict(n_classes=0), dict(n_classes=2.0), dict(n_classes=True),
               dict(class_names=["a", "b"]), dict(recording=[0]), dict(recording=[0.0, 1.0]), dict(class_id=[[0, 2]]), dict(start_s=["a", "b"]),
               dict(n_classes=4, class_names=["a", "b", "c"])):
        with pytest.raises(ValueError):
            Annotations(**{**ok, **kw})
    for name in ("recording", "start_s", "n_classes", "other"):               # immutable
        with pytest.raises(AttributeError):
            setattr(a, name, 1)
    with pytest.raises(AttributeError):
        del a.recording
    with pytest.raises(ValueError):
        a.start_s[0] = 3.0
    with pytest.raises(ValueError):
        a.reference_events(16000, 1)                                          # an annotation of recording 1, one recording
    with pytest.raises(ValueError):
        a.to_samples(0)


def test_to_samples_rounds_half_up():
    a = Annotations([0, 0, 0], [0, 0, 0], [0.0, 0.49, 0.5], [0.26, 1.5, 2.49], n_classes=1)
    lo, hi = a.to_samples(2)
    assert lo.dtype == np.int64 and lo.tolist() == [0, 1, 1] and hi.tolist() == [1, 3, 5]       # 0.52 -> 1, 0.98 -> 1, 1.0 -> 1; 4.98 -> 5
    assert a.to_samples(16000)[0].tolist() == A.to_samples(a.start_s, 16000).tolist() == [0, 7840, 8000]


def test_hand_worked_merges():
    #            overlapping       touching          nested              apart       another class over the same stretch, another recording
    rec = [0, 0, 0, 0, 0, 0, 0, 0, 1]
    cls = [0, 0, 0, 0, 0, 0, 0, 1, 0]
    start = [1.0, 1.5, 4.0, 5.0, 8.0, 8.5, 12.0, 1.0, 1.2]
    end = [2.0, 3.0, 5.0, 6.0, 11.0, 9.0, 13.0, 3.0, 1.4]
    a = Annotations(rec, cls, start, end, n_classes=3)
    ref = a.reference_events(10, 2)
    assert ref.lo.tolist() == [10, 40, 80, 120, 10, 12] and ref.hi.tolist() == [30, 60, 110, 130, 30, 14]
    assert ref.recording.tolist() == [0, 0, 0, 0, 0, 1] and ref.class_id.tolist() == [0, 0, 0, 0, 1, 0]
    assert ref.seg_offsets.tolist() == [0, 4, 5, 5, 6, 6, 6] and ref.prefix.tolist() == [0, 20, 40, 70, 80, 100, 102] and ref.n_ref.tolist() == [5, 1, 0]
    assert ref.lo.dtype == ref.hi.dtype == ref.seg_offsets.dtype == ref.prefix.dtype == ref.n_ref.dtype == np.int64
    assert a.reference_events(10, 2) is ref                                   # built once
    assert a.reference_events(10, 3).seg_offsets.tolist() == [0, 4, 5, 5, 6, 6, 6, 6, 6, 6]
    segs, table = A.reference_events(rec, cls, start, end, 10, 2, 3)
    assert segs[(0, 0)] == [(10, 30), (40, 60), (80, 110), (120, 130)] and segs[(0, 1)] == [(10, 30)] and segs[(1, 0)] == [(12, 14)] and segs[(1, 2)] == []
    for k in ("recording", "class_id", "lo", "hi", "seg_offsets", "prefix", "n_ref"):
        assert np.array_equal(getattr(ref, k), table[k]), k
    # given out of order, and with one annotation shorter than half a sample (it covers no sample)
    b = Annotations([0, 0, 0, 0], [0, 0, 0, 0], [5.0, 1.0, 2.0, 7.0], [6.0, 2.5, 3.0, 7.04], n_classes=1)
    assert b.reference_events(10).lo.tolist() == [10, 50] and b.reference_events(10).hi.tolist() == [30, 60] and b.reference_events(10).n_ref.tolist() == [2]
    with pytest.raises(ValueError):
        Annotations([0], [0], [0.0], [150000.0]).reference_events(16000)     # 2.4e9 samples in one event


def test_merge_matches_the_reference_on_random_input():
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(0, 40))
        rec, cls = rng.integers(0, 3, n), rng.integers(0, 4, n)
        start = rng.integers(0, 60, n) / 4.0
        end = start + rng.integers(1, 12, n) / 4.0
        ref = Annotations(rec, cls, start, end, n_classes=4).reference_events(4, 3)
        _, table = A.reference_events(rec, cls, start, end, 4, 3, 4)
        for k in ("recording", "class_id", "lo", "hi", "seg_offsets", "prefix", "n_ref"):
            assert np.array_equal(getattr(ref, k), table[k]), k


def test_hand_worked_cells():
    def cells(lengths, window_len, hop_len, tail="pad"):
        plan = WindowPlan(lengths, 16000, window_len, hop_len, tail)
        lo, hi = annotations.window_cells(plan)
        assert lo.dtype == hi.dtype == np.int64 and len(lo) == plan.n_windows
        want_lo, want_hi = [], []
        for (w0, w1), n in zip(plan.ranges, lengths):
            a, b = A.cells(plan.starts[w0:w1], n, window_len, hop_len)
            want_lo += a
            want_hi += b
        assert lo.tolist() == want_lo and hi.tolist() == want_hi
        return list(zip(lo.tolist(), hi.tolist()))

    assert cells([10], 4, 4) == [(0, 4), (4, 8), (8, 10)]                                          # hop = window: the windows themselves
    assert cells([10], 8, 3) == [(0, 5), (5, 8), (8, 10), (10, 10)]                                # 8 - 3 = 5 is odd: the shift is 2; an empty last cell
    assert cells([10], 8, 3, "drop") == [(0, 10)]
    assert cells([20], 4, 6) == [(0, 5), (5, 11), (11, 17), (17, 20)]                              # hop > window: (4 - 6) // 2 = -1, the gaps are owned too
    assert cells([10, 7], 4, 2) == [(0, 3), (3, 5), (5, 7), (7, 9), (9, 10), (0, 3), (3, 5), (5, 7), (7, 7)]
    assert cells([3], 16, 8) == [(0, 3)]                                                           # shorter than a window
    plan = WindowPlan([100, 37, 64], 16000, 16, 5)                                                 # cells partition every recording
    lo, hi = annotations.window_cells(plan)
    for (w0, w1), n in zip(plan.ranges, plan.n_samples):
        assert lo[w0] == 0 and hi[w1 - 1] == n and (lo[w0 + 1:w1] == hi[w0:w1 - 1]).all() and (hi[w0:w1] >= lo[w0:w1]).all()


def test_raven_round_trip(tmp_path):
    head = "Selection\tView\tChannel\tBegin Time (s)\tEnd Time (s)\tLow Freq (Hz)\tHigh Freq (Hz)\tSpecies\n"
    (tmp_path / "a.txt").write_text(head + "1\tSpectrogram 1\t1\t0.5\t1.25\t500\t4000\twren\n1\tWaveform 1\t1\t0.5\t1.25\t\t\twren\n"
                                    "2\tSpectrogram 1\t1\t3.0\t4.5\t500\t4000\tblackbird\n2\tWaveform 1\t1\t3.0\t4.5\t\t\tblackbird\n")
    (tmp_path / "b.txt").write_text(head + "1\tSpectrogram 1\t1\t10.0\t10.75\t200\t900\twren\n7\tSpectrogram 1\t1\t0.125\t0.25\t200\t900\towl\n")
    a = Annotations.from_raven([tmp_path / "a.txt", str(tmp_path / "b.txt")], class_column="Species")
    assert a.class_names == ("blackbird", "owl", "wren") and a.n_classes == 3
    assert a.recording.tolist() == [0, 0, 1, 1] and a.class_id.tolist() == [2, 0, 2, 1]           # the Waveform rows repeat their selections
    assert a.start_s.tolist() == [0.5, 3.0, 10.0, 0.125] and a.end_s.tolist() == [1.25, 4.5, 10.75, 0.25]
    b = Annotations.from_raven([tmp_path / "b.txt"], class_column="Species", recording=[4], class_names=["wren", "owl", "lark"])
    assert b.recording.tolist() == [4, 4] and b.class_id.tolist() == [0, 1] and b.n_classes == 3
    with pytest.raises(ValueError):
        Annotations.from_raven([tmp_path / "a.txt"], class_column="Species", class_names=["wren"])          # blackbird is not among them
    with pytest.raises(ValueError):
        Annotations.from_raven([tmp_path / "a.txt"], class_column="Call type")
    with pytest.raises(ValueError):
        Annotations.from_raven([tmp_path / "a.txt"], class_column="Species", recording=[0, 1])
    (tmp_path / "c.txt").write_text(head + "1\tSpectrogram 1\t1\tx\t1.0\t1\t2\twren\n")
    with pytest.raises(ValueError):
        Annotations.from_raven([tmp_path / "c.txt"], class_column="Species")
    # written back out and read again: the same annotations
    with open(tmp_path / "d.txt", "w") as f:
        f.write("Selection\tBegin Time (s)\tEnd Time (s)\tSpecies\n")
        for n, (c, s, e) in enumerate(zip(a.class_id[:2], a.start_s[:2], a.end_s[:2])):
            f.write(f"{n + 1}\t{float(s)!r}\t{float(e)!r}\t{a.class_names[c]}\n")
    d = Annotations.from_raven([tmp_path / "d.txt"], class_column="Species", class_names=a.class_names)
    assert d.class_id.tolist() == [2, 0] and d.start_s.tolist() == [0.5, 3.0] and d.end_s.tolist() == [1.25, 4.5]


def _disjoint(rng, n, top=60):
    """n disjoint intervals on 0 .. top in order, some touching, lengths 1 and up."""
    cuts = np.sort(rng.choice(np.arange(top + 1), size=2 * n, replace=False)) if n else np.zeros(0, dtype=np.int64)
    out = [(int(cuts[2 * k]), int(cuts[2 * k + 1])) for k in range(n)]
    for k in range(1, n):                                                     # close some gaps: touching intervals
        if rng.random() < 0.3:
            out[k] = (out[k - 1][1], out[k][1])
    return out


def test_walk_is_a_maximum_matching_and_the_scan_gives_its_pairs():
    """The claim the kernel design rests on, over 4 000 random cases with touching intervals and exact copies: compatible pairs never
    cross, a node has at most floor(1 / iou) partners, the walk has the cardinality of a maximum matching, and the in-order scan -- also
    as composed two-bit functions over chunks -- takes the walk's pairs."""
    rng = np.random.default_rng(22)
    multi = 0
    for case in range(4000):
        preds = _disjoint(rng, int(rng.integers(0, 9)))
        refs = _disjoint(rng, int(rng.integers(0, 9)))
        if preds and rng.random() < 0.3:                                       # exact copies of some predictions among the reference events
            keep = []
            for r in sorted(set(refs + [p for p in preds if rng.random() < 0.5])):
                if not keep or r[0] >= keep[-1][1]:
                    keep.append(r)
            refs = keep
        iou = IOUS[case % len(IOUS)]
        cp = A.compatible_pairs(preds, refs, iou)
        for (i1, j1) in cp:
            for (i2, j2) in cp:
                assert not (i1 < i2 and j1 > j2), (preds, refs, iou)
        deg_p, deg_r = np.bincount([i for i, _ in cp], minlength=9), np.bincount([j for _, j in cp], minlength=9)
        assert max(deg_p.max(), deg_r.max()) <= int(1 / iou) and len(cp) <= max(len(preds) + len(refs) - 1, 0)
        multi += int(max(deg_p.max(), deg_r.max()) > 1)
        w = A.walk(preds, refs, iou)
        assert len(w) == A.max_matching(preds, refs, iou), (preds, refs, iou)
        assert w == A.scan(preds, refs, iou) == A.scan_bytes(preds, refs, iou, chunk=1 + case % 5), (preds, refs, iou)
    assert multi > 300                                                        # the cases that can tell a greedy scan from a matching


def test_compatibility_at_exact_boundaries():
    # inter / union = 0.3: 3 of 10 samples.  fl(0.3) * 10.0 rounds to 3.0, so the exact ratio is compatible
    assert np.float64(0.3) * np.float64(10.0) == 3.0
    assert A.compatible((0, 8), (5, 10), 0.3) and not A.compatible((0, 7), (5, 10), 0.3) and A.compatible((0, 9), (5, 10), 0.3)
    assert not A.compatible((0, 8), (5, 11), 0.3)                             # 3 of 11
    # 0.5: 10 of 20
    assert A.compatible((0, 10), (0, 20), 0.5) and not A.compatible((0, 10), (0, 21), 0.5) and A.compatible((0, 10), (0, 19), 0.5)
    assert A.compatible((5, 15), (0, 20), 0.5) and not A.compatible((5, 14), (0, 20), 0.5)
    # 1: exact copies only
    assert A.compatible((3, 9), (3, 9), 1.0) and not A.compatible((3, 9), (3, 10), 1.0) and not A.compatible((4, 9), (3, 9), 1.0)
    # touching and disjoint intervals share no sample, whatever the threshold
    assert not A.compatible((0, 5), (5, 9), 1 / 16) and not A.compatible((0, 5), (7, 9), 1 / 16) and not A.compatible((4, 4), (0, 9), 1 / 16)
    assert A.compatible((0, 1), (0, 16), 1 / 16) and not A.compatible((0, 1), (0, 17), 1 / 16)
    # at the largest spans the products are still exact: 2^31 - 1 samples
    big = (1 << 31) - 1
    assert A.compatible((0, big), (0, big), 1.0) and not A.compatible((0, big), (1, big), 1.0) and not A.compatible((0, big), (1 << 30, big), 0.5)


def _declared(prefix):
    text = open(os.path.join(ROOT, "include", "avexhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


NAMES = ["avexhip_annot_chunk_pairs", "avexhip_annot_count", "avexhip_annot_match", "avexhip_annot_overlap", "avexhip_annot_workspace_bytes"]


def test_bindings(built_lib):
    assert _capi.header_abi_version() >= 22
    assert _declared("avexhip_annot_") == NAMES == sorted(n for n in _capi.SYMBOLS if n.startswith("avexhip_annot_"))
    for n in NAMES:
        assert hasattr(built_lib, n)
    from avex_amd import build
    assert "annotations.hip" in build.SOURCES
    text = open(os.path.join(ROOT, "include", "avexhip.h")).read()
    assert float(re.search(r"AVEXHIP_ANNOT_MIN_IOU ([0-9.]+)", text).group(1)) == annotations.MIN_IOU == 1 / 16
    assert int(re.search(r"AVEXHIP_ANNOT_CHUNK_PAIRS (\d+)", text).group(1)) == annotations.CHUNK_PAIRS == built_lib.avexhip_annot_chunk_pairs()
    # the struct as the header lays it out
    body = re.search(r"typedef struct \{([^}]*)\} avexhip_annot_match_args;", text).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in _capi.AnnotMatchArgs._fields_] and C.sizeof(_capi.AnnotMatchArgs) == 18 * 8 + 8


def test_workspace_is_a_function_of_the_three_counts(built_lib):
    f = built_lib.avexhip_annot_workspace_bytes
    assert len(_capi.SYMBOLS["avexhip_annot_workspace_bytes"][1]) == 3                             # n_pred, n_ref, n_segments: no windows, no classes apart

    def want(p, a):
        up = lambda n: (n + 15) // 16 * 16
        nch = (p + a + 255) // 256
        return 2 * up(4 * p) + 2 * up(4 * (p + a)) + 2 * up(nch)

    for p, a, s in ((1, 1, 1), (7, 300, 3), (1 << 20, 1 << 20, 1), (1 << 20, 1 << 20, 512 * 32), (1000, 5, 99)):
        assert f(p, a, s) == want(p, a), (p, a, s)
    assert f(1 << 20, 1 << 20, 1) < 40 << 20
    for p, a, s in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1 << 31, 1, 1), (1 << 30, 1 << 30, 1), (1, 1, 1 << 31)):
        assert f(p, a, s) == 0, (p, a, s)


def test_argument_checks_need_no_gpu(built_lib):
    """Each entry point refuses a bad call before it touches the device; the pointers below are never dereferenced."""
    lib, fake = built_lib, 1 << 20
    seg = np.array([0, 2, 2, 3, 3], dtype=np.int64)                           # 2 recordings x 2 classes, 3 events
    win_rec = np.array([0, 0, 1], dtype=np.int32)

    def overlap(**kw):
        a = dict(lo=fake, hi=fake, wr=win_rec, wr_dev=fake, n_win=3, n_rec=2, c=2, seg=seg, seg_dev=fake, rlo=fake, rhi=fake, pre=fake, n_ref=3, out=fake)
        a.update(kw)
        return lib.avexhip_annot_overlap(a["lo"], a["hi"], a["wr"].ctypes.data if a["wr"] is not None else None, a["wr_dev"], a["n_win"], a["n_rec"], a["c"],
                                         a["seg"].ctypes.data if a["seg"] is not None else None, a["seg_dev"], a["rlo"], a["rhi"], a["pre"], a["n_ref"], a["out"], None)

    for kw, word in ((dict(lo=None), "null"), (dict(wr=None), "null"), (dict(seg=None), "null"), (dict(pre=None), "null"), (dict(out=None), "null"),
                     (dict(hi=fake + 4), "aligned"), (dict(out=fake + 2), "aligned"), (dict(n_win=0), "n_win"), (dict(n_rec=0), "n_rec"), (dict(c=0), "n_classes"),
                     (dict(n_ref=0), "n_ref"), (dict(n_ref=4), "not n_ref"), (dict(seg=np.array([1, 2, 2, 3, 3], dtype=np.int64)), "not 0"),
                     (dict(seg=np.array([0, 2, 1, 3, 3], dtype=np.int64)), "seg_offsets[2]"), (dict(wr=np.array([0, 2, 1], dtype=np.int32)), "window 1"),
                     (dict(wr=np.array([-1, 0, 1], dtype=np.int32)), "window 0"), (dict(n_win=1 << 31, c=1), "n_win")):
        assert overlap(**kw) == -1 and word in _capi.last_error(), (kw, _capi.last_error())

    ws_bytes = lib.avexhip_annot_workspace_bytes(5, 3, 4)

    def args(**kw):
        v = dict(sequence=fake, class_id=fake, first=fake, last=fake, n_pred=5, cell_lo=fake, cell_hi=fake, n_windows=9, seg_offsets_host=seg.ctypes.data,
                 seg_offsets_dev=fake, ref_lo=fake, ref_hi=fake, n_ref=3, iou=0.5, workspace=fake, workspace_bytes=ws_bytes, counts=fake, errors=fake, n_rec=2,
                 n_classes=2)
        v.update(kw)
        a = _capi.AnnotMatchArgs()
        for k, x in v.items():
            setattr(a, k, x)
        return a

    bad_seg = np.array([0, 2, 2, 3, 4], dtype=np.int64)
    cases = ((dict(first=None), "null"), (dict(cell_hi=None), "null"), (dict(seg_offsets_host=None), "null"), (dict(workspace=None), "null"), (dict(counts=None), "null"),
             (dict(errors=None), "null"), (dict(last=fake + 2), "aligned"), (dict(counts=fake + 4), "aligned"), (dict(workspace=fake + 8), "aligned"),
             (dict(n_pred=0), "n_pred"), (dict(n_ref=0), "n_ref"), (dict(n_pred=1 << 31), "n_pred"), (dict(n_windows=0), "n_windows"), (dict(n_rec=0), "n_rec"),
             (dict(n_classes=-1), "n_classes"), (dict(iou=0.06), "iou"), (dict(iou=1.0001), "iou"), (dict(iou=float("nan")), "iou"),
             (dict(seg_offsets_host=bad_seg.ctypes.data), "not n_ref"), (dict(n_rec=3), "seg_offsets"))
    for kw, word in cases:
        assert lib.avexhip_annot_count(C.byref(args(**kw)), None) == -1 and word in _capi.last_error(), (kw, _capi.last_error())
        assert lib.avexhip_annot_match(C.byref(args(**kw)), fake, fake, fake, None) == -1 and word in _capi.last_error(), (kw, _capi.last_error())
    for fn in (lambda a: lib.avexhip_annot_count(C.byref(a), None), lambda a: lib.avexhip_annot_match(C.byref(a), fake, fake, fake, None)):
        assert fn(args(workspace_bytes=ws_bytes - 1)) == -4 and "workspace" in _capi.last_error()
    assert lib.avexhip_annot_count(None, None) == -1 and "null" in _capi.last_error()
    for ptrs, word in (((None, fake, fake), "null"), ((fake, None, fake), "null"), ((fake, fake, None), "null"), ((fake + 4, fake, fake), "aligned"),
                       ((fake, fake + 2, fake), "aligned")):
        assert lib.avexhip_annot_match(C.byref(args()), *ptrs, None) == -1 and word in _capi.last_error(), (ptrs, _capi.last_error())


def _pred(first, last, cls, seq=None):
    n = len(first)
    return {"sequence": torch.tensor(seq if seq is not None else [0] * n, dtype=torch.int32), "class_id": torch.tensor(cls, dtype=torch.int32),
            "first": torch.tensor(first, dtype=torch.int32), "last": torch.tensor(last, dtype=torch.int32), "peak": torch.zeros(n)}


def test_python_argument_checks_come_before_the_device():
    plan = WindowPlan([64], 16000, 8, 4)
    ann = Annotations([0], [0], [0.0], [0.001])
    pred = _pred([0], [1], [0])
    with pytest.raises(TypeError):
        annotations.window_overlap(plan, "ann")
    with pytest.raises(TypeError):
        annotations.window_overlap(object(), ann)
    with pytest.raises(ValueError):
        annotations.window_overlap(plan, ann, span="hull")
    for kw in (dict(min_overlap_s=-1.0), dict(min_overlap_s=float("nan")), dict(min_fraction=0.0), dict(min_fraction=1.5), dict(min_fraction=1e-5),
               dict(min_fraction=True), dict(span="x")):
        with pytest.raises(ValueError):
            annotations.window_labels(plan, ann, **kw)
    for iou in (0.0, 0.06, 1.01, float("nan"), True, "0.5"):
        with pytest.raises(ValueError):
            annotations.match_events(pred, ann, plan, iou=iou)
    with pytest.raises(ValueError):
        annotations.match_events({"first": pred["first"]}, ann, plan)
    with pytest.raises(ValueError):
        annotations.match_events({**pred, "last": pred["last"].long()}, ann, plan)
    with pytest.raises(ValueError):
        annotations.match_events({**pred, "last": torch.zeros(2, dtype=torch.int32)}, ann, plan)
    with pytest.raises(ValueError):
        annotations.score_events(pred, Annotations([1], [0], [0.0], [0.001]), plan)               # recording 1 of one
    scores = np.zeros((plan.n_windows, 1), dtype=np.float32)
    for kw in (dict(thresholds=[]), dict(thresholds=[0.5, float("nan")]), dict(thresholds=[[0.5]]), dict(thresholds=[0.5], off_ratio=0.0),
               dict(thresholds=[0.5], off_ratio=1.5), dict(thresholds=[0.5], iou=2.0)):
        with pytest.raises(ValueError):
            annotations.sweep_thresholds(scores, plan, ann, **kw)
    with pytest.raises(TypeError):
        annotations.sweep_thresholds(scores, plan, ann, [0.5], on=0.3)
    assert annotations._label_rules(16000, 0.01, 0.3) == (160, annotations.Fraction(3, 10)) and annotations._label_rules(16000, None, None) == (1, None)
    assert annotations._label_rules(16000, 0.0, 1 / 3)[1] == annotations.Fraction(1, 3) and annotations._label_rules(10, 0.26, None)[0] == 3


def test_class_sums_over_more_than_one_block():
    """The per-class float64 sums behind average_precision (plain torch, so they run here): rows sorted by bucket, buckets of 0, 1, 4096,
    4097 and 10 000 rows, against fsum.  n terms in [0, 1] summed in any order stay within n^2 2^-53 of the exact sum."""
    import math
    rng = np.random.default_rng(4)
    sizes = [4097, 0, 1, 4096, 10000, 0]
    bucket = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes))
    local = torch.from_numpy(np.concatenate([np.arange(n) for n in sizes]))
    term = rng.random(sum(sizes)) * (rng.random(sum(sizes)) < 0.7)
    got = annotations._class_sums(torch.from_numpy(term), bucket, local, torch.tensor(sizes))
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(sizes),)
    at = 0
    for c, n in enumerate(sizes):
        assert abs(float(got[c]) - math.fsum(term[at:at + n])) <= n * n * 2.0 ** -53, c
        at += n
    assert got[1] == 0.0 and got[2] == term[4097]
    assert torch.equal(got, annotations._class_sums(torch.from_numpy(term), bucket, local, torch.tensor(sizes)))


def test_no_cpu_fallback(built_lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    plan = WindowPlan([64], 16000, 8, 4)
    ann = Annotations([0], [0], [0.0], [0.001])
    pred = _pred([0], [1], [0])
    for call in (lambda: annotations.window_overlap(plan, ann), lambda: annotations.window_classes(plan, ann), lambda: annotations.match_events(pred, ann, plan),
                 lambda: annotations.score_events(pred, ann, plan), lambda: annotations.score_windows(pred, ann, plan),
                 lambda: annotations.sweep_thresholds(np.zeros((plan.n_windows, 1), dtype=np.float32), plan, ann, [0.5])):
        with pytest.raises(_capi.AvexHipError):
            call()


def test_public_names_and_signatures():
    for name in ("Annotations", "score_events", "sweep_thresholds"):
        assert name in avex_amd.__all__ and getattr(avex_amd, name) is getattr(annotations, name)
    sig = lambda f: str(inspect.signature(f))
    assert sig(Annotations.__init__).startswith("(self, recording, class_id, start_s, end_s, *, n_classes") and "class_names" in sig(Annotations.__init__)
    p = inspect.signature(Annotations.from_raven).parameters
    assert list(p) == ["paths", "class_column", "recording", "class_names"] and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    assert list(inspect.signature(annotations.window_cells).parameters) == ["windows"]
    for fn, lead, kw in ((annotations.window_overlap, ["windows", "annotations"], {"span": "window"}),
                         (annotations.window_labels, ["windows", "annotations"], {"span": "window", "min_overlap_s": None, "min_fraction": None}),
                         (annotations.window_classes, ["windows", "annotations"], {"span": "window", "min_overlap_s": None, "min_fraction": None}),
                         (annotations.match_events, ["pred", "annotations", "windows"], {"iou": 0.5}),
                         (annotations.score_events, ["pred", "annotations", "windows"], {"iou": 0.5}),
                         (annotations.score_windows, ["pred", "annotations", "windows"], {"min_overlap_s": None, "min_fraction": None})):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + list(kw), fn.__name__
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == v for k, v in kw.items()), fn.__name__
    p = inspect.signature(annotations.sweep_thresholds).parameters
    assert list(p) == ["scores", "windows", "annotations", "thresholds", "off_ratio", "iou", "row_of_window", "rules"]
    assert p["off_ratio"].default == 1.0 and p["iou"].default == 0.5 and p["row_of_window"].default is None and p["rules"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(annotations.report).parameters) == ["result", "class_names"]
