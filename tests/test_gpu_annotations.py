"""Annotations and detection scoring on the GPU against tests/_annotations_ref.py: every integer output equal bit for bit.

Matching cases are laid out on a plan with hop = window = 4 samples, so window k owns the cell [4 k, 4 k + 4) and an event (first, last)
spans [4 first, 4 last + 4); reference events are given in seconds at 16 kHz, where s / 16000 goes back to s exactly."""
import numpy as np
import pytest
import torch

import _annotations_ref as A
from avex_amd import _capi, annotations
from avex_amd.annotations import Annotations, WindowPlan

pytestmark = pytest.mark.gpu

SR = 16000
CELL = 4
IOUS = (1 / 16, 0.3, 0.5, 0.75, 1.0)
INT_KEYS = ("n_pred", "n_ref", "tp", "fp", "fn")
RATIO_KEYS = ("precision", "recall", "f1", "micro_precision", "micro_recall", "micro_f1")


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _pred(rows, peaks=None, capacity=None):
    """[(sequence, class, first, last)] -> the columns of a decode on the device; rows past the events are filler, as decode_events leaves them."""
    n = len(rows)
    cap = n if capacity is None else capacity
    cols = np.full((4, cap), -1, dtype=np.int32)
    if n:
        cols[:, :n] = np.asarray(rows, dtype=np.int32).T
    peak = np.full(cap, -np.inf, dtype=np.float32)
    peak[:n] = np.zeros(n, dtype=np.float32) if peaks is None else peaks
    out = {k: _dev(cols[i], torch.int32) for i, k in enumerate(("sequence", "class_id", "first", "last"))}
    out["peak"] = _dev(peak, torch.float32)
    out["count"] = torch.tensor(n, dtype=torch.int64, device="cuda")
    return out


def _rows_of(pred):
    return [tuple(int(pred[k][i]) for k in ("sequence", "class_id", "first", "last")) for i in range(pred["first"].shape[0])]


class Case:
    """Predictions (in cells) and reference events (in samples) per (recording, class), on a plan of 4-sample cells."""

    def __init__(self, n_rec, n_classes, cells_per_rec):
        self.n_rec, self.n_classes = n_rec, n_classes
        self.plan = WindowPlan([cells_per_rec * CELL] * n_rec, SR, CELL, CELL)
        self.preds, self.refs = {}, {}

    def pred(self, r, c, first, last):
        self.preds.setdefault((r, c), []).append((first, last))

    def ref(self, r, c, lo, hi):
        self.refs.setdefault((r, c), []).append((lo, hi))

    def rows(self):
        out = []
        for (r, c) in sorted(self.preds):
            w0 = self.plan.ranges[r][0]
            out += [(r, c, w0 + f, w0 + l) for f, l in sorted(self.preds[(r, c)])]
        return out

    def annotations(self):
        flat = [(r, c, lo, hi) for (r, c), ev in sorted(self.refs.items()) for lo, hi in ev]
        return Annotations([x[0] for x in flat], [x[1] for x in flat], [x[2] / SR for x in flat], [x[3] / SR for x in flat], n_classes=self.n_classes)

    def table(self, ann):
        return A.reference_events(ann.recording, ann.class_id, ann.start_s, ann.end_s, SR, self.n_rec, self.n_classes)[1]


def _check_match(case, iou, rows=None, capacity=None):
    """match_events against the reference walk; returns the device result and the reference arrays."""
    ann = case.annotations()
    table = case.table(ann)
    rows = case.rows() if rows is None else rows
    lo, hi = annotations.window_cells(case.plan)
    want_p, want_r, spans = A.match(rows, lo, hi, table, case.n_classes, iou)
    got = annotations.match_events(_pred(rows, capacity=capacity), ann, case.plan, iou=iou)
    assert int(got["order_errors"]) == 0
    assert got["match_of_pred"].dtype == got["match_of_ref"].dtype == torch.int32
    assert np.array_equal(got["match_of_pred"].cpu().numpy()[:len(rows)], want_p), iou
    assert (got["match_of_pred"].cpu().numpy()[len(rows):] == -1).all()
    assert np.array_equal(got["match_of_ref"].cpu().numpy(), want_r), iou
    assert got["pred_lo"].cpu().tolist()[:len(rows)] == [s[0] for s in spans] and got["pred_hi"].cpu().tolist()[:len(rows)] == [s[1] for s in spans]
    return got, want_p, want_r


# ---------------------------------------------------------------------------------------------------------------------------- overlap
def _overlap_setup(n_classes):
    lengths = [150001, 97003, 80000]
    plan = WindowPlan(lengths, SR, 400, 160)                                   # shift (400 - 160) // 2 = 120; 938 + 607 + 500 windows
    assert plan.n_windows == 2045
    rng = np.random.default_rng(100 + n_classes)
    rec, cls, lo, hi = [], [], [], []

    def add(r, c, a, b):
        rec.append(r); cls.append(c); lo.append(a); hi.append(b)

    add(0, 0, 160 * 50 + 300, 160 * 50 + 400)                                  # 100 samples: a quarter of windows 50 and 51 exactly
    add(0, 0, 160 * 90 + 10, 160 * 90 + 109)                                   # 99 samples wholly inside window 90
    add(0, 0, 160 * 200, 160 * 210)                                            # from a window's first sample to another's, over several windows
    add(0, 0, 160 * 210, 160 * 211 + 400)                                      # touches the one before (they merge), ends at a window's end
    add(0, 0, 160 * 300 + 7, 160 * 300 + 8)                                    # one sample
    add(0, 0, 149990, 150001)                                                  # up to the last sample of the recording
    add(2, 0, 0, 80000)                                                        # a whole recording
    for c in range(1, n_classes):                                              # recording 1 has no annotation at all; some classes have none either
        if c % 3 == 2:
            continue
        for r in (0, 2):
            for _ in range(int(rng.integers(0, 6))):
                a = int(rng.integers(0, lengths[r] - 2000))
                add(r, c, a, a + int(rng.integers(1, 2000)))
    ann = Annotations(rec, cls, np.asarray(lo) / SR, np.asarray(hi) / SR, n_classes=n_classes)
    segs, _ = A.reference_events(rec, cls, np.asarray(lo) / SR, np.asarray(hi) / SR, SR, 3, n_classes)
    return plan, ann, segs


@pytest.mark.parametrize("n_classes", [1, 3, 65])
def test_overlap_labels_and_classes(n_classes):
    plan, ann, segs = _overlap_setup(n_classes)
    spans = {"window": (plan.starts, plan.starts + plan.valids), "cell": annotations.window_cells(plan)}
    for span, (lo, hi) in spans.items():
        want = A.overlap(lo, hi, plan.recording, segs, n_classes)
        got = annotations.window_overlap(plan, ann, span=span)
        assert got.dtype == torch.int32 and tuple(got.shape) == (plan.n_windows, n_classes) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), span
        assert (want[plan.ranges[1][0]:plan.ranges[1][1]] == 0).all() and want[plan.ranges[2][0]:, 0].tolist() == (hi - lo)[plan.ranges[2][0]:].tolist()
        length = (hi - lo).astype(np.int64)[:, None]
        for kw, rule in ((dict(), want >= 1), (dict(min_overlap_s=100 / SR), want >= 100), (dict(min_fraction=0.25), (want >= 1) & (want.astype(np.int64) * 4 >= length)),
                         (dict(min_overlap_s=0.004, min_fraction=1 / 3), (want >= 64) & (want.astype(np.int64) * 3 >= length))):
            labels = annotations.window_labels(plan, ann, span=span, **kw)
            assert labels.dtype == torch.bool and np.array_equal(labels.cpu().numpy(), rule), (span, kw)
            n_lab = rule.sum(1)
            want_cls = np.where(n_lab == 1, rule.argmax(1), np.where(n_lab == 0, -1, -2)).astype(np.int32)
            got_cls = annotations.window_classes(plan, ann, span=span, **kw)
            assert got_cls.dtype == torch.int32 and np.array_equal(got_cls.cpu().numpy(), want_cls), (span, kw)
    # the boundaries the rules were placed on: exactly a quarter of a window (labelled) and one sample less (not)
    want = A.overlap(*spans["window"], plan.recording, segs, n_classes)
    assert want[50, 0] == 100 and want[51, 0] == 100 and want[90, 0] == 99 and want[49, 0] == 0 and want[300, 0] == 1
    quarter = annotations.window_labels(plan, ann, min_fraction=0.25).cpu().numpy()
    assert quarter[50, 0] and quarter[51, 0] and not quarter[90, 0] and not quarter[300, 0]
    assert want[200:212, 0].tolist() == [400] * 12 and want[197:200, 0].tolist() == [0, 80, 240] and want[212:215, 0].tolist() == [240, 80, 0]


def test_overlap_without_annotations_is_zero():
    plan = WindowPlan([1000], SR, 100, 50)
    got = annotations.window_overlap(plan, Annotations([], [], [], [], n_classes=2), span="cell")
    assert tuple(got.shape) == (plan.n_windows, 2) and int(got.abs().sum()) == 0
    assert annotations.window_classes(plan, Annotations([], [], [], [], n_classes=2)).cpu().tolist() == [-1] * plan.n_windows


# --------------------------------------------------------------------------------------------------------------------------- matching
PERIOD, LENGTH = 16, 15           # cells: intervals of 60 samples every 64; shifted by half a period they share 28 of 92 samples = 0.304


def _chain(case, r, c, n_pred, n_ref, first_cell=0, lead_ref=False):
    """A staggered chain: prediction i over cells [16 i, 16 i + 14], reference event j half a period later (lead_ref: one more in front)."""
    for i in range(n_pred):
        case.pred(r, c, first_cell + PERIOD * i, first_cell + PERIOD * i + LENGTH - 1)
    for j in range(-1 if lead_ref else 0, n_ref):
        lo = (first_cell + PERIOD * j) * CELL + PERIOD * CELL // 2
        case.ref(r, c, lo, lo + LENGTH * CELL)


def test_a_staggered_chain_over_scan_chunks_and_the_same_chain_less_its_head():
    """One segment, 400 + 400 intervals, 799 compatible pairs at 0.3: more than three scan chunks.  As built every prediction i takes
    reference event i; without the first prediction every prediction i takes event i - 1: each later decision flips, so a carry that is
    wrong at any chunk boundary shows."""
    n = 400
    case = Case(1, 1, PERIOD * (n + 2))
    _chain(case, 0, 0, n, n)
    rows = case.rows()
    lo, hi = annotations.window_cells(case.plan)
    table = case.table(case.annotations())
    spans = [(int(lo[f]), int(hi[l])) for _, _, f, l in rows]
    refs = list(zip(table["lo"].tolist(), table["hi"].tolist()))
    assert len(A.compatible_pairs(spans, refs, 0.3)) == 2 * n - 1 >= 3 * annotations.CHUNK_PAIRS
    _, want_p, _ = _check_match(case, 0.3)
    assert want_p.tolist() == list(range(n))
    _, want_p, want_r = _check_match(case, 0.3, rows=rows[1:])
    assert want_p.tolist() == list(range(n - 1)) and want_r.tolist() == list(range(n - 1)) + [-1]
    for iou in (0.5, 1.0):                                                     # 0.304 is not enough: nothing matches
        _, want_p, _ = _check_match(case, iou)
        assert (want_p == -1).all()


def test_a_chain_that_crosses_a_segment_boundary_at_a_chunk_boundary():
    """Segment (0, 0) holds exactly 256 pairs, so segment (0, 1)'s first pair opens the second chunk with the first chain's last state in the
    carry: a new prediction and a new reference event, which must reset it."""
    case = Case(1, 2, PERIOD * 140)
    _chain(case, 0, 0, 128, 128, first_cell=PERIOD, lead_ref=True)            # 129 reference events: 2 * 128 pairs
    _chain(case, 0, 1, 100, 100)
    lo, hi = annotations.window_cells(case.plan)
    table = case.table(case.annotations())
    spans = [(int(lo[f]), int(hi[l])) for _, c, f, l in case.rows() if c == 0]
    refs = list(zip(table["lo"][:129].tolist(), table["hi"][:129].tolist()))
    assert table["seg_offsets"].tolist() == [0, 129, 229] and len(A.compatible_pairs(spans, refs, 0.3)) == annotations.CHUNK_PAIRS
    _, want_p, want_r = _check_match(case, 0.3)
    assert want_p[:128].tolist() == list(range(128)) and want_r[128] == -1 and want_p[128:].tolist() == list(range(129, 229))


def test_more_scan_chunks_than_one_pass_of_the_carry():
    """1 024 segments (classes) that each hold the same staggered chain of 33 predictions, every second one with a reference event in
    front: 512 * 65 + 512 * 66 compatible pairs, more than 256 scan chunks, so the one workgroup that carries the state over the chunk
    functions takes a second pass and carries a composed state into it -- inside a chain, where a wrong state flips every later
    decision of the segment.  (One segment of each kind is counted with compatible_pairs; all of a kind are copies.)"""
    n, n_seg = 33, 1024
    case = Case(1, n_seg, PERIOD * (n + 2))
    for c in range(n_seg):
        _chain(case, 0, c, n, n, first_cell=PERIOD, lead_ref=c % 2 == 1)
    rows = case.rows()
    lo, hi = annotations.window_cells(case.plan)
    table = case.table(case.annotations())
    per_kind = []
    for c in (0, 1):
        spans = [(int(lo[f]), int(hi[l])) for _, cc, f, l in rows if cc == c]
        a, b = table["seg_offsets"][c:c + 2].tolist()
        per_kind.append(len(A.compatible_pairs(spans, list(zip(table["lo"][a:b].tolist(), table["hi"][a:b].tolist())), 0.3)))
    assert per_kind == [2 * n - 1, 2 * n]
    total = n_seg // 2 * sum(per_kind)
    assert total > 256 * annotations.CHUNK_PAIRS and (256 * annotations.CHUNK_PAIRS) % sum(per_kind) not in (0, per_kind[0])      # the pass boundary is inside a chain
    _, want_p, want_r = _check_match(case, 0.3)
    assert (want_p >= 0).all() and (want_r == -1).sum() == n_seg // 2          # every prediction matched; the last event of a chain with a lead is left over


def _mixed_case():
    """Every shape of segment in one call: stars both ways, exact copies, zero-length predictions, segments with only predictions, only
    reference events or neither, and many short segments that share a chunk."""
    case = Case(40, 3, 64)
    # recording 0, class 0: one prediction over three reference events (0.33, 0.33, 0.32 of it), then the mirror image
    case.pred(0, 0, 0, 24)
    for lo, hi in ((0, 33), (34, 67), (68, 100)):
        case.ref(0, 0, lo, hi)
    for f, l in ((30, 37), (39, 46), (48, 55)):                                # 32 samples each of the event's 104
        case.pred(0, 0, f, l)
    case.ref(0, 0, 120, 224)
    # recording 0, class 1: exact copies, one of them a single cell; a near copy one sample short
    for f, l in ((2, 5), (7, 7), (10, 19)):
        case.pred(0, 1, f, l)
        case.ref(0, 1, f * CELL, (l + 1) * CELL - (1 if f == 10 else 0))
    # recording 0, class 2: predictions only; recording 1, class 0: reference events only; recording 1, class 1: neither
    case.pred(0, 2, 3, 9)
    case.pred(0, 2, 20, 20)
    case.ref(1, 0, 8, 40)
    case.ref(1, 0, 100, 140)
    # recording 1, class 2: a prediction over sixteen events too short for it (7 of 128 samples is below 1/16), then two touching
    # predictions that each hold half of one event (4 of 12 samples)
    case.pred(1, 2, 0, 31)
    for k in range(16):
        case.ref(1, 2, 8 * k, 8 * k + 7)
    case.pred(1, 2, 32, 33)
    case.pred(1, 2, 34, 35)
    case.ref(1, 2, 132, 140)
    # recordings 2 .. 39: short segments, one or two events a side, at shifts that land on both sides of every threshold
    rng = np.random.default_rng(7)
    for r in range(2, 40):
        for c in range(3):
            kind = int(rng.integers(0, 5))
            if kind == 0:
                continue
            pos = 0
            for _ in range(int(rng.integers(1, 3))):
                f = pos + int(rng.integers(0, 4))
                l = f + int(rng.integers(0, 8))
                if l >= 60:
                    break
                if kind != 1:
                    case.pred(r, c, f, l)
                if kind != 2:
                    a = max(f * CELL + int(rng.integers(-6, 7)), pos * CELL)
                    b = max((l + 1) * CELL + int(rng.integers(-6, 7)), a + 1)
                    case.ref(r, c, a, min(b, 63 * CELL))
                pos = l + 3
    return case


@pytest.mark.parametrize("iou", IOUS)
def test_every_shape_of_segment(iou):
    case = _mixed_case()
    rows = case.rows()
    got, want_p, want_r = _check_match(case, iou, capacity=len(rows) + 37)    # filler rows behind count
    by_row = dict(zip(rows, want_p.tolist()))
    w1 = case.plan.ranges[1][0]
    if iou == 0.3:
        assert by_row[(0, 0, 0, 24)] == 0 and [by_row[(0, 0, f, l)] for f, l in ((30, 37), (39, 46), (48, 55))] == [3, -1, -1]      # the stars: first come
    if iou == 1.0:
        assert [by_row[(0, 1, f, l)] for f, l in ((2, 5), (7, 7), (10, 19))] == [4, 5, -1] and int((want_p >= 0).sum()) >= 2      # exact copies only
    if iou <= 0.3:
        assert by_row[(1, 2, w1 + 32, w1 + 33)] == 25 and by_row[(1, 2, w1 + 34, w1 + 35)] == -1                                   # a third of the union each: the first takes it
    assert by_row[(1, 2, w1, w1 + 31)] == -1 and by_row[(0, 2, 3, 9)] == -1 and by_row[(0, 2, 20, 20)] == -1 and want_r[7:9].tolist() == [-1, -1]


def test_sixteen_partners_at_the_lowest_threshold():
    case = Case(1, 1, 64)
    case.pred(0, 0, 0, 31)                                                     # 128 samples
    for k in range(16):
        case.ref(0, 0, 8 * k, 8 * k + 7 + (k == 15))                           # 7 samples (below 1/16 of 128), the last one 8: exactly 1/16
    case.pred(0, 0, 40, 40)
    _, want_p, want_r = _check_match(case, 1 / 16)
    assert want_p.tolist() == [15, -1] and want_r.tolist() == [-1] * 15 + [0]
    case = Case(1, 1, 64)
    case.ref(0, 0, 0, 128)
    for k in range(16):
        case.pred(0, 0, 2 * k, 2 * k + 1)                                      # sixteen predictions of 8 samples: each exactly 1/16 of the event
    _, want_p, want_r = _check_match(case, 1 / 16)
    assert want_p.tolist() == [0] + [-1] * 15 and want_r.tolist() == [0]


def test_zero_length_predictions_match_nothing():
    plan = WindowPlan([10, 10], SR, 8, 3)                                      # cells (0, 5) (5, 8) (8, 10) (10, 10) per recording: the last one is empty
    lo, hi = annotations.window_cells(plan)
    assert (lo[3], hi[3]) == (10, 10)
    ann = Annotations([0, 1], [0, 0], [0.0, 8 / SR], [10 / SR, 10 / SR], n_classes=1)
    rows = [(0, 0, 0, 2), (0, 0, 3, 3), (1, 0, 7, 7)]
    got = annotations.match_events(_pred(rows), ann, plan, iou=1 / 16)
    assert got["match_of_pred"].cpu().tolist() == [0, -1, -1] and got["match_of_ref"].cpu().tolist() == [0, -1] and int(got["order_errors"]) == 0
    assert got["pred_lo"].cpu().tolist() == [0, 10, 10] and got["pred_hi"].cpu().tolist() == [10, 10, 10]


def test_no_predictions_or_no_reference_events():
    case = _mixed_case()
    ann = case.annotations()
    for cap in (0, 5):
        s = annotations.score_events(_pred([], capacity=cap), ann, case.plan)
        assert s["tp"].cpu().tolist() == [0, 0, 0] and s["fn"].cpu().tolist() == s["n_ref"].cpu().tolist() == case.table(ann)["n_ref"].tolist()
        assert (s["match_of_ref"] == -1).all() and tuple(s["match_of_pred"].shape) == (cap,) and int(s["order_errors"]) == 0
        assert torch.isnan(s["precision"]).all() and s["recall"].cpu().tolist() == [0.0, 0.0, 0.0]
    rows = case.rows()
    s = annotations.score_events(_pred(rows), Annotations([], [], [], [], n_classes=3), case.plan)
    assert s["fp"].cpu().tolist() == s["n_pred"].cpu().tolist() == np.bincount([c for _, c, _, _ in rows], minlength=3).tolist()
    assert (s["match_of_pred"] == -1).all() and s["match_of_ref"].numel() == 0 and torch.isnan(s["recall"]).all() and torch.isnan(s["average_precision"]).all()
    assert int(s["order_errors"]) == 0


def test_the_same_bits_on_every_run_and_from_a_larger_buffer():
    case = _mixed_case()
    _chain(case, 39, 2, 300, 300)                                              # and a chain of 599 pairs behind the short segments
    case.plan = WindowPlan([PERIOD * 302 * CELL] * 40, SR, CELL, CELL)
    ann, rows = case.annotations(), case.rows()
    peaks = np.random.default_rng(3).random(len(rows)).astype(np.float32)
    runs = [annotations.score_events(_pred(rows, peaks, capacity=cap), ann, case.plan, iou=0.3) for cap in (None, None, len(rows) + 1000)]
    _check_match(case, 0.3)
    for other in runs[1:]:
        assert torch.equal(runs[0]["match_of_pred"], other["match_of_pred"][:len(rows)]) and torch.equal(runs[0]["match_of_ref"], other["match_of_ref"])
        for k in INT_KEYS + RATIO_KEYS:
            assert torch.equal(runs[0][k].view(torch.int64), other[k].view(torch.int64)), k
        assert torch.equal(runs[0]["iou_of_pred"].view(torch.int64), other["iou_of_pred"][:len(rows)].view(torch.int64))
    assert torch.isnan(runs[2]["iou_of_pred"][len(rows):]).all()


def test_out_of_order_input_is_reported_and_stays_in_bounds():
    case = _mixed_case()
    ann, rows = case.annotations(), case.rows()
    n_ref = len(case.table(ann)["lo"])
    swapped = list(rows)
    swapped[0], swapped[3] = swapped[3], swapped[0]                            # within one segment
    moved = rows[5:] + rows[:5]                                                # whole segments out of place
    overlapping = [rows[0], (0, 0, 10, 30)] + rows[1:]                         # not disjoint
    behind_filler = [rows[0], (-1, -1, -1, -1)] + rows[1:]
    outside = [rows[0], (0, 3, 40, 41), (40, 0, 1, 2), (0, 1, 50, 70000), (0, 1, 9, 8)] + rows[1:]
    for bad in (swapped, moved, overlapping, behind_filler, outside):
        s = annotations.score_events(_pred(bad), ann, case.plan, iou=0.3)
        assert int(s["order_errors"]) >= 1
        mop, mor = s["match_of_pred"].cpu().numpy(), s["match_of_ref"].cpu().numpy()
        assert mop.shape == (len(bad),) and mor.shape == (n_ref,) and mop.min() >= -1 and mop.max() < n_ref and mor.min() >= -1 and mor.max() < len(bad)
        with pytest.raises(_capi.AvexHipError):
            annotations.report(s)
    assert int(annotations.score_events(_pred(outside), ann, case.plan)["order_errors"]) == 4
    good = annotations.report(annotations.score_events(_pred(rows), ann, case.plan, iou=0.3), class_names=["a", "b", "c"])
    assert good["order_errors"] == 0 and set(good["per_class"]) == {"a", "b", "c"} and good["per_class"]["a"]["tp"] == int(good["tp"][0])


# ----------------------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("iou", [0.3, 0.5])
def test_scores_against_the_reference(iou):
    case = _mixed_case()
    _chain(case, 39, 2, 60, 60)
    case.plan = WindowPlan([PERIOD * 62 * CELL] * 40, SR, CELL, CELL)
    ann, rows = case.annotations(), case.rows()
    table = case.table(ann)
    peaks = np.round(np.random.default_rng(11).random(len(rows)), 1).astype(np.float32)          # ties: the event number breaks them
    lo, hi = annotations.window_cells(case.plan)
    want_p, want_r, spans = A.match(rows, lo, hi, table, 3, iou)
    want = A.scores(rows, peaks, want_p, table, 3)
    got = annotations.score_events(_pred(rows, peaks, capacity=len(rows) + 9), ann, case.plan, iou=iou)
    for k in INT_KEYS:
        assert got[k].dtype == torch.int64 and got[k].cpu().tolist() == want[k].tolist(), k
    for k in RATIO_KEYS:                                                       # one correctly rounded division of the same integers
        assert got[k].dtype == torch.float64 and np.array_equal(got[k].cpu().numpy(), want[k], equal_nan=True), k
    for k in ("macro_precision", "macro_recall", "macro_f1"):                 # a mean of three numbers in [0, 1], summed in an order torch chooses
        assert abs(float(got[k]) - want[k]) <= 3 * 2.0 ** -53, k
    ap = got["average_precision"].cpu().numpy()
    for c in range(3):
        bound = float(want["n_pred"][c]) ** 2 * 2.0 ** -53 / float(want["n_ref"][c])             # n terms in [0, 1], each sum correctly rounded
        print(f"class {c}: AP {ap[c]!r} against {want['average_precision'][c]!r}, bound {bound:.3e} ({want['n_pred'][c]} predictions, {want['n_ref'][c]} events)")
        assert bound < 1e-11 and abs(ap[c] - want["average_precision"][c]) <= bound
    assert int((want_p >= 0).sum()) >= 50 and 0.0 < want["average_precision"][2] < 1.0
    iou_got = got["iou_of_pred"].cpu().numpy()
    for i, j in enumerate(want_p):
        if j >= 0:
            assert iou_got[i] == A.iou_of(spans[i], (int(table["lo"][j]), int(table["hi"][j]))) >= iou
        else:
            assert np.isnan(iou_got[i])
    assert np.isnan(iou_got[len(rows):]).all()


def test_scores_of_a_class_larger_than_a_sum_block():
    """5 000 predictions of one class (more than one block of the per-class sums) beside a small class, ranked by distinct peaks."""
    n = 5000
    case = Case(1, 2, PERIOD * (n + 2))
    _chain(case, 0, 0, n, n)
    case.refs[(0, 0)] = [r for j, r in enumerate(case.refs[(0, 0)]) if j % 3 != 1]       # holes in the chain: fewer events than predictions
    for k in range(0, 40, 2):
        case.pred(0, 1, 5 * k, 5 * k + 3)
        case.ref(0, 1, 20 * k + (k % 3) * CELL, 20 * k + 16)                   # exact, 3/4 and 1/2 of the prediction in turn
    ann, rows = case.annotations(), case.rows()
    table = case.table(ann)
    peaks = np.random.default_rng(12).permutation(len(rows)).astype(np.float32)
    rows = [r for i, r in enumerate(rows) if i % 7 != 3]                       # drop predictions here and there: the chain's matches flip back and forth
    peaks = peaks[:len(rows)]
    lo, hi = annotations.window_cells(case.plan)
    want_p, want_r, _ = A.match(rows, lo, hi, table, 2, 0.3)
    want = A.scores(rows, peaks, want_p, table, 2)
    got = annotations.score_events(_pred(rows, peaks), ann, case.plan, iou=0.3)
    assert np.array_equal(got["match_of_pred"].cpu().numpy(), want_p) and np.array_equal(got["match_of_ref"].cpu().numpy(), want_r)
    for k in INT_KEYS:
        assert got[k].cpu().tolist() == want[k].tolist(), k
    assert want["n_pred"][0] > 4096 and 0 < want["tp"][0] < want["n_pred"][0] and 0 < want["tp"][1] < 20
    ap = got["average_precision"].cpu().numpy()
    for c in range(2):
        bound = float(want["n_pred"][c]) ** 2 * 2.0 ** -53 / float(want["n_ref"][c])
        print(f"class {c}: AP {ap[c]!r} against {want['average_precision'][c]!r}, bound {bound:.3e}")
        assert bound < 1e-12 and abs(ap[c] - want["average_precision"][c]) <= bound


# ------------------------------------------------------------------------------------------------------------------------- end to end
def _planted():
    """Two recordings of 20 s and 10 s in windows of 1 s every 0.5 s: window i of a recording owns [0.5 i + 0.25, 0.5 i + 0.75) s (the first
    from 0, the last to the end).  Runs of scores (recording, class, first, last, score) and annotations (recording, class, start_s, end_s)."""
    plan = WindowPlan([20 * SR, 10 * SR], SR, SR, SR // 2)
    assert plan.n_windows == 60 and plan.ranges == [(0, 40), (40, 60)]
    runs = [(0, 0, 4, 7, 0.9),        # 2.25 .. 4.25 s, annotated exactly: IoU 1
            (0, 0, 20, 23, 0.6),      # 10.25 .. 12.25 s, annotated 0.5 s late: 1.5 / 2.5 = 0.6
            (0, 0, 30, 31, 0.4),      # a decoy below the planted threshold
            (0, 1, 10, 11, 0.9),      # 5.25 .. 6.25 s, annotated 6.0 .. 7.0: 0.25 / 1.75, a miss and a false alarm
            (1, 0, 1, 2, 0.9),        # no annotation: a false alarm
            (1, 1, 5, 9, 0.6),        # 2.75 .. 5.25 s, annotated exactly
            (1, 1, 14, 15, 0.4)]      # a decoy
    ann = Annotations([0, 0, 0, 1, 1], [0, 0, 1, 1, 0], [2.25, 10.75, 6.0, 2.75, 7.0], [4.25, 12.75, 7.0, 5.25, 8.0], n_classes=2, class_names=["chirp", "trill"])
    scores = np.full((60, 2), 0.2, dtype=np.float32)
    for r, c, f, l, v in runs:
        scores[plan.ranges[r][0] + f:plan.ranges[r][0] + l + 1, c] = v
    return plan, ann, torch.from_numpy(scores).cuda()


def test_end_to_end_decode_score_sweep():
    from avex_amd.detection import decode_events
    plan, ann, scores = _planted()
    pred = decode_events(scores, windows=plan, on=0.5)
    assert _rows_of(pred) == [(0, 0, 4, 7), (0, 0, 20, 23), (0, 1, 10, 11), (1, 0, 41, 42), (1, 1, 45, 49)]
    s = annotations.report(annotations.score_events(pred, ann, plan), ann.class_names)
    assert s["n_pred"].tolist() == [3, 2] and s["n_ref"].tolist() == [3, 2] and s["tp"].tolist() == [2, 1] and s["fp"].tolist() == [1, 1] and s["fn"].tolist() == [1, 1]
    assert s["match_of_pred"].tolist() == [0, 1, -1, -1, 4] and s["match_of_ref"].tolist() == [0, 1, -1, -1, 4]      # events: (0,0) x2, (0,1), (1,0), (1,1)
    assert s["iou_of_pred"][:2].tolist() == [1.0, 0.6] and s["iou_of_pred"][4] == 1.0 and np.isnan(s["iou_of_pred"][2:4]).all()
    assert s["precision"].tolist() == [2 / 3, 0.5] and s["recall"].tolist() == [2 / 3, 0.5] and s["f1"].tolist() == [4 / 6, 0.5]
    assert s["micro_f1"] == 6 / 10 and s["per_class"]["trill"]["fn"] == 1
    assert s["average_precision"].tolist() == [(1 / 1 + 2 / 3) / 3, (1 / 2) / 2]                  # ranked 0.9, 0.9 (a miss), 0.6 / 0.9 (a miss), 0.6
    # at IoU 0.75 the late annotation is lost
    assert annotations.score_events(pred, ann, plan, iou=0.75)["tp"].cpu().tolist() == [1, 1]
    # the window-level counterpart: cells that hold a marked sample against the events' windows
    w = annotations.report(annotations.score_windows(pred, ann, plan))
    labels = annotations.window_labels(plan, ann, span="cell").cpu().numpy()
    predicted = np.zeros((60, 2), dtype=bool)
    for _, c, f, l in _rows_of(pred):
        predicted[f:l + 1, c] = True
    assert np.array_equal(w["predicted"], predicted) and np.array_equal(w["labels"], labels)
    assert labels[:, 0].nonzero()[0].tolist() == [4, 5, 6, 7, 21, 22, 23, 24, 53, 54, 55] and w["tp"].tolist() == [7, 6] and w["fp"].tolist() == [3, 1]
    assert w["fn"].tolist() == [4, 2] and w["tn"].tolist() == [46, 51] and w["precision"].tolist() == [0.7, 6 / 7]

    thresholds = [0.7, 0.1, 0.5, 0.95, 0.3]
    sweep = annotations.sweep_thresholds(scores, plan, ann, thresholds, max_events=16)
    assert sweep["best_threshold"].cpu().tolist() == [0.5, 0.5] and tuple(sweep["f1"].shape) == (5, 2) and int(sweep["order_errors"]) == 0
    for t, th in enumerate(thresholds):
        one = annotations.score_events(decode_events(scores, windows=plan, on=th, off=th, max_events=16), ann, plan)
        for k in INT_KEYS + ("precision", "recall", "f1", "average_precision", "micro_f1", "macro_f1"):
            assert torch.equal(torch.nan_to_num(sweep[k][t], nan=-1.0), torch.nan_to_num(one[k], nan=-1.0)), (th, k)
    assert sweep["f1"].cpu()[:, 0].tolist() == [2 / 5, 0.0, 4 / 6, 0.0, 4 / 7]                    # 0.7: one of two found; 0.1: one event a recording; 0.3: a decoy more
    tie = annotations.sweep_thresholds(scores, plan, ann, [0.55, 0.45, 0.5], off_ratio=0.9)
    assert tie["best_threshold"].cpu().tolist() == [0.45, 0.45]                                   # the same events at all three: the lowest wins


def test_window_classes_feed_an_example_bank():
    from avex_amd.examples import ExampleBank
    plan, ann, _ = _planted()
    labels = annotations.window_classes(plan, ann, span="cell", min_fraction=0.5).cpu()
    assert labels[[4, 7, 10, 12, 13, 0]].tolist() == [0, 0, -1, 1, 1, -1] and int((labels == -2).sum()) == 0
    emb = torch.randn(plan.n_windows, 32, generator=torch.Generator().manual_seed(0)).cuda()
    sel = labels >= -1
    bank = ExampleBank(32, n_classes=2)
    added = bank.add(emb[sel.cuda()], labels[sel])
    assert len(added) == int(sel.sum()) and bank.counts.tolist() == [int((labels == 0).sum()), int((labels == 1).sum()), int((labels == -1).sum())]
    top = bank.score(emb[4:5]).argmax(dim=1)
    assert int(top[0]) == 0
