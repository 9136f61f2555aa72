"""avex_amd.search without a GPU: the NumPy restatement against hand-written cases, the ABI 15 bindings and struct layouts, the
workspace size, the refusals of the entry points, and every ValueError of the Python layer."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _search_ref as S
from avex_amd import _capi, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMS = ("avexhip_search_max_k", "avexhip_search_workspace_bytes", "avexhip_search_prepare_rows", "avexhip_search_begin", "avexhip_search_chunk",
        "avexhip_search_finish")


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_prepared_rows():
    x = np.array([[3.0, 4.0], [0.0, 0.0], [1.0, -1.0]], dtype=np.float32)
    p = S.prepared(x, "cosine")
    assert p.dtype == np.float32 and p[0].tolist() == [np.float32(0.6), np.float32(0.8)] and p[1].tolist() == [0.0, 0.0]      # a zero row stays zero
    assert np.array_equal(S.prepared(x, "dot"), x) and S.prepared(x, "dot") is not x
    with pytest.raises(ValueError):
        S.prepared(x, "euclidean")


def test_topk_order_ties_nan_and_short_sets():
    sim = np.array([0.5, 1.0, 0.5, np.nan, -0.0, 0.0, 1.0], dtype=np.float32)
    s, r, c = S.topk_from_sim(sim, 4)
    assert r.tolist() == [1, 6, 0, 2] and s.tolist() == [1.0, 1.0, 0.5, 0.5] and c == 4                 # ties broken by the lower row
    s, r, c = S.topk_from_sim(sim, 10)                                                                      # k > rows: the NaN is gone, the tail is -1 / -inf
    assert c == 6 and r.tolist() == [1, 6, 0, 2, 4, 5, -1, -1, -1, -1] and np.isneginf(s[6:]).all()
    assert not np.signbit(s[4]) and not np.signbit(s[5])                                                    # -0.0 ties with, and is returned as, +0.0
    s, r, c = S.topk_from_sim(sim, 3, skip_row=1)
    assert r.tolist() == [6, 0, 2]
    s, r, c = S.topk_from_sim(sim, 3, skip_row=1, excluded=np.array([1, 0, 0, 0, 0, 0, 1], dtype=bool))
    assert r.tolist() == [2, 4, 5] and c == 3
    s, r, c = S.topk_from_sim(np.array([np.nan, np.nan], dtype=np.float32), 2)
    assert c == 0 and r.tolist() == [-1, -1]
    s, r, c = S.topk_from_sim(np.array([-np.inf, np.inf, -1.0], dtype=np.float32), 3)                      # infinities are ordered like numbers
    assert r.tolist() == [1, 2, 0] and c == 3 and s.dtype == np.float32 and r.dtype == np.int64


def test_nms_hand_written_cases():
    #          row:   0     1     2     3     4     5
    rec = np.array([0, 0, 0, 1, -1, -1], dtype=np.int32)
    start = np.array([0.0, 1.0, 0.5, 0.0, 0.0, 0.0])
    end = np.array([1.0, 2.0, 1.5, 1.0, 1.0, 1.0])
    order = [0, 1, 2, 3, 4, 5]
    # rows 0 and 1 only touch: both survive at max_overlap 0; row 2 overlaps both by half: falls at 0 and at 0.25, survives at 0.5
    assert S.nms(order, rec, start, end, 0.0, 6) == [0, 1, 3, 4, 5]
    assert S.nms(order, rec, start, end, 0.25, 6) == [0, 1, 3, 4, 5]
    assert S.nms(order, rec, start, end, 0.5, 6) == [0, 1, 2, 3, 4, 5]                                      # 0.5 > 0.5 * 1.0 is false
    # the same spans in another recording, or in none, never suppress and are never suppressed (rows 3, 4, 5 equal row 0's span)
    assert S.nms([4, 0, 5, 3], rec, start, end, 0.0, 4) == [0, 1, 2, 3]
    # it stops at k kept hits
    assert S.nms(order, rec, start, end, 0.0, 2) == [0, 1] and S.nms([0, 2, 1], rec, start, end, 0.0, 2) == [0, 2]
    # the shorter of the two sets the bound: a 0.25 s window inside a 1 s one overlaps by its whole length
    rec2, st2, en2 = np.zeros(2, dtype=np.int32), np.array([0.0, 0.25]), np.array([1.0, 0.5])
    assert S.nms([0, 1], rec2, st2, en2, 0.9, 2) == [0] and S.nms([1, 0], rec2, st2, en2, 0.9, 2) == [0]
    # fewer than k survivors: five windows of one recording, hop = window / 4, at max_overlap 0 every second pair still overlaps
    rec3 = np.zeros(5, dtype=np.int32)
    st3 = np.arange(5) * 0.25
    assert S.nms([0, 1, 2, 3, 4], rec3, st3, st3 + 1.0, 0.0, 5) == [0, 4]


def test_search_restatement_applies_nms_over_the_overfetched_list():
    rec = np.zeros(6, dtype=np.int32)
    start = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 5.0])
    sim = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.1]], dtype=np.float32)
    r = S.search(sim, 2, nms_overlap=0.0, overfetch=2, rec=rec, start=start, end=start + 1.0)             # K' = 4: row 4 is never seen
    assert r["rows"].tolist() == [[0, -1]] and r["count"].tolist() == [1] and np.isneginf(r["scores"][0, 1]) and np.isnan(r["start_s"][0, 1])
    r = S.search(sim, 2, nms_overlap=0.0, overfetch=3, rec=rec, start=start, end=start + 1.0)             # K' = 6
    assert r["rows"].tolist() == [[0, 4]] and r["start_s"].tolist() == [[0.0, 1.0]] and r["end_s"].tolist() == [[1.0, 2.0]] and r["recording"].tolist() == [[0, 0]]
    r = S.search(sim, 600, nms_overlap=0.0, overfetch=4, rec=rec, start=start, end=start + 1.0)           # K' = min(2400, 1024)
    assert r["count"].tolist() == [3] and r["rows"][0, :3].tolist() == [0, 4, 5]


def test_exclusion_masks():
    rec = np.array([0, 0, 0, 1, -1], dtype=np.int32)
    start = np.array([0.0, 1.0, 0.5, 0.5, 0.5])
    end = start + 1.0
    assert S.exclude_mask(None, 0, 0.0, 1.0, rec, start, end).tolist() == [False] * 5
    assert S.exclude_mask("recording", 0, 0.0, 1.0, rec, start, end).tolist() == [True, True, True, False, False]
    assert S.exclude_mask("recording", -1, 0.0, 1.0, rec, start, end).tolist() == [False] * 5             # a query without a recording excludes nothing
    assert S.exclude_mask("overlap", 0, 0.0, 1.0, rec, start, end).tolist() == [True, False, True, False, False]      # row 1 only touches
    assert S.exclude_mask("overlap", 1, 0.0, 1.0, rec, start, end).tolist() == [False, False, False, True, False]
    assert S.exclude_mask("overlap", 0, 3.0, 4.0, rec, start, end).tolist() == [False] * 5


def test_a_nan_span_takes_part_in_nothing():
    """np.minimum / np.maximum carry a NaN and every compare with it is false: a row with a recording but no span is not excluded by
    "overlap", excludes nothing as a query, and neither suppresses nor is suppressed."""
    rec = np.zeros(4, dtype=np.int32)
    start = np.array([0.0, np.nan, 0.25, np.nan])
    end = np.array([1.0, np.nan, 1.25, np.nan])
    assert S.exclude_mask("overlap", 0, 0.0, 1.0, rec, start, end).tolist() == [True, False, True, False]
    assert S.exclude_mask("overlap", 0, np.nan, np.nan, rec, start, end).tolist() == [False] * 4
    assert S.exclude_mask("recording", 0, np.nan, np.nan, rec, start, end).tolist() == [True] * 4
    assert S.nms([0, 1, 2, 3], rec, start, end, 0.0, 4) == [0, 1, 3]                                        # row 2 falls to row 0 alone
    assert S.nms([1, 0, 3, 2], rec, start, end, 0.0, 4) == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------------------ the bindings
def test_bindings(built_lib):
    assert _capi.header_abi_version() >= 15
    for name in SYMS:
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name
    hdr = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/avexhip.h").read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(avexhip_search_[a-z0-9_]+)\s*\(", hdr))) == sorted(SYMS)
    assert built_lib.avexhip_search_max_k() == 1024 == search.MAX_K


def test_search_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of the ABI 15 structs as gcc sees include/avexhip.h == the ctypes mirrors."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    structs = {"avexhip_search_args": _capi.SearchArgs, "avexhip_search_result": _capi.SearchResult}
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


def test_workspace_is_monotone_and_knows_no_database_size(built_lib):
    ws = built_lib.avexhip_search_workspace_bytes
    assert len(_capi.SYMBOLS["avexhip_search_workspace_bytes"][1]) == 4                                     # chunk_rows, d, batch, k: no n_db
    base = (4096, 768, 256, 100)
    b0 = ws(*base)
    # at least the similarities of one batch against one chunk, the prepared queries and the lists
    assert b0 >= 4 * 256 * 4096 + 4 * 256 * 768 + 8 * 256 * 100
    assert b0 <= 2 * (4 * 256 * 4096 + 4 * 256 * 768 + 8 * 256 * 100)
    for axis, steps in enumerate(((1, 63, 64, 65, 4096, 65536, 1 << 20), (1, 31, 32, 33, 768, 4096), (1, 2, 255, 256, 1024, 4096), (1, 2, 100, 1023, 1024))):
        sizes = []
        for v in steps:
            a = list(base)
            a[axis] = v
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], (axis, sizes)
    for bad in ((0, 768, 256, 100), (4096, 0, 256, 100), (4096, 768, 0, 100), (4096, 768, 256, 0), (4096, 768, 256, 1025), (1 << 31, 768, 256, 100)):
        assert ws(*bad) == 0, bad


def _args(**kw):
    fake = 1 << 20                                                        # a 16-byte aligned number: never dereferenced, the call is refused first
    a = _capi.SearchArgs()
    a.query, a.ld_query, a.nb, a.d, a.batch, a.k, a.chunk_rows, a.normalise = fake, 64, 4, 64, 8, 10, 256, 1
    a.chunk, a.row0, a.n_rows = fake, 0, 256
    a.workspace, a.workspace_bytes = fake, 1 << 30
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _result(**kw):
    fake = 1 << 20
    r = _capi.SearchResult()
    r.k, r.nms, r.max_overlap, r.n_rows = 10, 0, 0.0, 256
    for name in ("scores", "rows", "count", "recording", "start_s", "end_s"):
        setattr(r, name, fake)
    for key, v in kw.items():
        setattr(r, key, v)
    return r


def test_entry_points_refuse_bad_shapes(built_lib):
    """rc -1 and a message that names the offending number, before the device is touched."""
    fake = 1 << 20
    lib = built_lib

    def refused(rc, *words):
        msg = _capi.last_error()
        assert rc == -1, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    refused(lib.avexhip_search_prepare_rows(fake, 10, 5, 64, 1, fake, None), "search_prepare_rows", "ld_rows 10")
    refused(lib.avexhip_search_prepare_rows(fake, 64, -1, 64, 1, fake, None), "n -1")
    refused(lib.avexhip_search_prepare_rows(fake, 64, 5, 0, 1, fake, None), "d 0")
    refused(lib.avexhip_search_prepare_rows(fake, 64, 5, 64, 2, fake, None), "normalise 2")
    refused(lib.avexhip_search_prepare_rows(None, 64, 5, 64, 1, fake, None), "null")
    for fn, name in ((lib.avexhip_search_begin, "search_begin"), (lib.avexhip_search_chunk, "search_chunk")):
        refused(fn(C.byref(_args(k=1025)), None), name, "k 1025")
        refused(fn(C.byref(_args(k=0)), None), name, "k 0")
        refused(fn(C.byref(_args(nb=9)), None), name, "nb 9")
        refused(fn(C.byref(_args(nb=0)), None), name, "nb 0")
        refused(fn(C.byref(_args(d=0)), None), name, "d 0")
        refused(fn(C.byref(_args(chunk_rows=0)), None), name, "chunk_rows 0")
        refused(fn(C.byref(_args(workspace=None)), None), name, "null")
    refused(lib.avexhip_search_begin(C.byref(_args(ld_query=63)), None), "ld_query 63")
    refused(lib.avexhip_search_begin(C.byref(_args(normalise=3)), None), "normalise 3")
    refused(lib.avexhip_search_chunk(C.byref(_args(n_rows=257)), None), "257 rows")
    refused(lib.avexhip_search_chunk(C.byref(_args(n_rows=0)), None), "0 rows")
    refused(lib.avexhip_search_chunk(C.byref(_args(row0=-1)), None), "-1")
    refused(lib.avexhip_search_chunk(C.byref(_args(row0=(1 << 31) - 256)), None), str((1 << 31) - 256))      # the last row would be 2^31 - 1
    refused(lib.avexhip_search_chunk(C.byref(_args(exclude=3)), None), "exclude 3")
    refused(lib.avexhip_search_chunk(C.byref(_args(exclude=1)), None), "exclude 1", "recordings")
    refused(lib.avexhip_search_chunk(C.byref(_args(exclude=2, query_recording=fake, db_recording=fake)), None), "spans")
    refused(lib.avexhip_search_chunk(C.byref(_args(stages=4)), None), "stages 4")
    refused(lib.avexhip_search_chunk(C.byref(_args(sim_out=fake, ld_sim=255)), None), "ld_sim 255")
    rc = lib.avexhip_search_chunk(C.byref(_args(workspace_bytes=1000)), None)                                 # a workspace too small has its own code
    assert rc == -4 and "1000 B" in _capi.last_error()
    assert lib.avexhip_search_begin(C.byref(_args(workspace_bytes=1000)), None) == -4
    fin = lib.avexhip_search_finish
    refused(fin(C.byref(_args()), C.byref(_result(k=11)), None), "search_finish", "k 11")
    refused(fin(C.byref(_args()), C.byref(_result(k=0)), None), "k 0")
    refused(fin(C.byref(_args()), C.byref(_result(k=5)), None), "k 5")                                        # fewer hits than the lists hold: only with suppression
    refused(fin(C.byref(_args()), C.byref(_result(k=5, nms=1, max_overlap=1.0)), None), "max_overlap 1")
    refused(fin(C.byref(_args()), C.byref(_result(k=5, nms=1, max_overlap=-0.5)), None), "max_overlap -0.5")
    refused(fin(C.byref(_args()), C.byref(_result(nms=2)), None), "nms 2")
    refused(fin(C.byref(_args()), C.byref(_result(n_rows=-1)), None), "-1 rows")
    refused(fin(C.byref(_args()), C.byref(_result(scores=None)), None), "null")
    refused(fin(C.byref(_args()), C.byref(_result(db_recording=fake)), None), "spans")
    refused(fin(C.byref(_args(k=2000)), C.byref(_result()), None), "k 2000")
    assert fin(C.byref(_args(workspace_bytes=1000)), C.byref(_result()), None) == -4


# ------------------------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture()
def no_gpu(monkeypatch):
    """Whatever reaches the device fails the test: every ValueError below is raised before _capi.require_gpu()."""
    def boom():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_capi, "require_gpu", boom)


def _filled(dim=8, n=5):
    """An index that claims n rows without having touched a device (searches are refused before they look at them)."""
    ix = search.EmbeddingIndex(dim)
    ix._n = n
    ix.names = ["a", "b"]
    return ix


def test_constructor_errors(no_gpu):
    for bad in (dict(dim=0), dict(dim=-3), dict(dim=2.5), dict(dim=8, metric="euclidean"), dict(dim=8, metric=None), dict(dim=8, chunk_rows=0),
                dict(dim=8, chunk_rows=1 << 31), dict(dim=8, chunk_rows=1.5)):
        with pytest.raises(ValueError):
            search.EmbeddingIndex(**bad)
    ix = search.EmbeddingIndex(8, metric="dot", chunk_rows=128)
    assert len(ix) == 0 and ix.n_recordings == 0 and ix.names == [] and ix.dpad == 32 and ix.metric == "dot"


def test_add_errors(no_gpu):
    ix = search.EmbeddingIndex(8)
    x = np.zeros((4, 8), dtype=np.float32)
    for bad in (np.zeros((4, 7), dtype=np.float32), np.zeros((8,), dtype=np.float32), torch.zeros(4, 8, 1), np.zeros((4, 9))):
        with pytest.raises(ValueError):
            ix.add(bad)
    with pytest.raises(ValueError):
        ix.add(x, recording=[0, 0, 0])                                    # metadata of the wrong length
    with pytest.raises(ValueError):
        ix.add(x, recording=0, start_s=np.zeros(4), end_s=np.zeros(5))
    with pytest.raises(ValueError):
        ix.add(x, recording=0, start_s=np.zeros((4, 1)), end_s=np.zeros(4))
    with pytest.raises(ValueError):
        ix.add(x, recording=0, start_s=np.zeros(4))                       # one end of the span without the other
    with pytest.raises(ValueError):
        ix.add_recording({"embeddings": torch.zeros(3, 8), "start_s": np.zeros(4), "end_s": np.zeros(4)})
    with pytest.raises(ValueError):
        ix.add_recording({"embeddings": [torch.zeros(4, 8)], "start_s": np.zeros(4), "end_s": np.zeros(4)})
    assert ix.add(np.zeros((0, 8), dtype=np.float32)) == range(0, 0) and len(ix) == 0
    big = _filled(8, (1 << 31) - 2)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        big.add(np.zeros((2, 8), dtype=np.float32))                       # one row more than 2^31 - 1
    with pytest.raises(ValueError):
        search.EmbeddingIndex.from_recordings(None, ["a.wav"], 1.0, metric="l2")
    with pytest.raises(ValueError):
        search.EmbeddingIndex.from_recordings(None, ["a.wav", "b.wav"], 1.0, names=["a"])


def test_search_errors(no_gpu):
    ix = _filled()
    q = np.zeros((3, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="empty"):
        search.EmbeddingIndex(8).search(q)
    with pytest.raises(ValueError, match="empty"):
        search.EmbeddingIndex(8).search_rows([0])
    for bad_q in (np.zeros((3, 7), dtype=np.float32), np.zeros(8, dtype=np.float32), torch.zeros(3, 9)):
        with pytest.raises(ValueError):
            ix.search(bad_q)
    for kw in (dict(k=0), dict(k=1025), dict(k=-1), dict(k=2.0), dict(k=True), dict(overfetch=0), dict(overfetch=1.5), dict(nms=1.0), dict(nms=-0.1),
               dict(nms="0.5"), dict(nms=True), dict(exclude="self"), dict(exclude="Recording"), dict(batch_size=0), dict(batch_size=-4)):
        with pytest.raises(ValueError):
            ix.search(q, **kw)
        with pytest.raises(ValueError):
            ix.search_rows([0, 1], **kw)
        with pytest.raises(ValueError):
            search.query_by_example(None, ix, np.zeros(16000, dtype=np.float32), **kw)
    with pytest.raises(ValueError, match="query_recording"):
        ix.search(q, exclude="recording")
    with pytest.raises(ValueError, match="query_recording"):
        ix.search(q, exclude="overlap", query_start_s=0.0, query_end_s=1.0)
    with pytest.raises(ValueError, match="query_start_s"):
        ix.search(q, exclude="overlap", query_recording=0)
    with pytest.raises(ValueError, match="query_start_s"):
        ix.search(q, exclude="overlap", query_recording=0, query_start_s=0.0)
    with pytest.raises(ValueError):
        ix.search(q, exclude="recording", query_recording=[0, 1])         # three queries, two ids
    with pytest.raises(ValueError):
        ix.search(q, exclude="overlap", query_recording=0, query_start_s=np.zeros(3), query_end_s=np.zeros(2))
    with pytest.raises(ValueError):
        ix.search(q, exclude="recording", query_recording="c")            # no recording of that name
    for bad_rows in ([5], [-1], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            ix.search_rows(bad_rows)
    with pytest.raises(ValueError, match="empty"):
        search.query_by_example(None, search.EmbeddingIndex(8), np.zeros(16000, dtype=np.float32))


def test_state_dict_errors_and_signature(no_gpu):
    st = {"rows": np.zeros((3, 7), dtype=np.float32), "recording": np.zeros(3, dtype=np.int32), "start_s": np.zeros(3), "end_s": np.zeros(3),
          "names": np.asarray(["a"]), "metric": np.asarray("cosine"), "dim": np.asarray(8), "chunk_rows": np.asarray(128)}
    with pytest.raises(ValueError):
        search.EmbeddingIndex.from_state_dict(st)                         # rows narrower than dim
    st["rows"] = np.zeros((3, 8), dtype=np.float32)
    st["end_s"] = np.zeros(2)
    with pytest.raises(ValueError):
        search.EmbeddingIndex.from_state_dict(st)
    st["end_s"], st["metric"] = np.zeros(3), np.asarray("l2")
    with pytest.raises(ValueError):
        search.EmbeddingIndex.from_state_dict(st)
    empty = search.EmbeddingIndex(8, metric="dot", chunk_rows=64).state_dict()                             # an empty index round-trips without a device
    assert empty["rows"].shape == (0, 8) and str(empty["metric"]) == "dot"
    back = search.EmbeddingIndex.from_state_dict(empty)
    assert len(back) == 0 and back.metric == "dot" and back.chunk_rows == 64 and back.dim == 8
    sig = inspect.signature(search.EmbeddingIndex.search)
    assert [p for p in sig.parameters][:3] == ["self", "query", "k"] and sig.parameters["k"].default == 10 and sig.parameters["overfetch"].default == 4
    assert sig.parameters["batch_size"].default == 1024 and sig.parameters["nms"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(search.EmbeddingIndex.search_rows).parameters["exclude"].default == "overlap"
    assert inspect.signature(search.EmbeddingIndex.__init__).parameters["chunk_rows"].default == 65536
    import avex_amd
    assert avex_amd.EmbeddingIndex is search.EmbeddingIndex and avex_amd.query_by_example is search.query_by_example
