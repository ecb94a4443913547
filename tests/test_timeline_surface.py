"""CPU checks of the timeline evidence's surface: the header's declaration, the library's export, the ctypes
table, the Python keywords and the timeline.csv writer (no GPU needed)."""
import csv
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO


def test_header_declares_the_entry():
    text = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mr_windows_timeline\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 19 and args[-1].startswith("int32_t* status") and args[17].startswith("int64_t* tl_out")
    assert [a.rsplit(" ", 1)[0] for a in args[7:18]] == ["const int32_t*", "const int32_t*", "int32_t", "int", "const int64_t*",
                                                         "const int64_t*", "int32_t", "int64_t*", "int64_t*", "int64_t*",
                                                         "int64_t*"]
    assert [a.rsplit(" ", 1)[1] for a in args[10:14]] == ["what", "b0", "bw", "B"]
    doc = re.sub(r"[\s*]+", " ", text[text.index("timeline evidence"):text.index("int mr_windows_timeline")])
    for word in ("T11", "T2", "mr_op_latency", "before", "after", "(uint64)tstart - (uint64)b0", "bitwise reproducible",
                 "MR_ERR_STATE", "tested in this order", "no fallback", "THAT RANK", "1..512"):
        assert word in doc, word


def test_library_exports_the_entry():
    from microrank_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mr_windows_timeline")


def test_signature():
    from microrank_amd import _lib
    from microrank_amd._lib import P, i32p, i64p

    vpp = C.POINTER(C.c_void_p)
    assert _lib.SIGNATURES["mr_windows_timeline"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int, i64p, i64p, C.c_int32,
                  i64p, i64p, i64p, i64p, i32p])


def _params(fn):
    return inspect.signature(fn).parameters


def _positional(fn):
    return [p.name for p in _params(fn).values() if p.kind != p.KEYWORD_ONLY]


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import online_rca as o

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank):
        p = _params(fn)["timeline"]
        assert p.kind == p.KEYWORD_ONLY and p.default is None, fn.__name__
    for fn in (o.windows_timeline, o.window_timeline):
        p = _params(fn)
        assert p["buckets"].kind == p["buckets"].KEYWORD_ONLY and p["buckets"].default == 30
        assert p["what"].kind == p["what"].KEYWORD_ONLY and p["what"].default == "self"
    assert _positional(o.windows_timeline) == ["ctx", "windows", "ops"]
    assert [n for n, p in _params(o.windows_timeline).items() if p.kind == p.KEYWORD_ONLY] == ["buckets", "what", "origin",
                                                                                               "width"]
    assert _params(o.windows_timeline)["origin"].default is None and _params(o.windows_timeline)["width"].default is None
    assert _positional(o.window_timeline) == _positional(o.window_calls) == ["data", "start_time", "end_time", "slo", "ops"]
    assert [n for n, p in _params(o.window_timeline).items() if p.kind == p.KEYWORD_ONLY] == ["buckets", "what", "ctx",
                                                                                              "table", "dev"]
    # the positional names of the existing entries are what they were
    assert _positional(o.rca_window) == ["data", "start_time", "end_time", "slo"]
    assert _positional(o.rank_windows) == ["ctx", "windows"]
    assert _positional(o.online_anomaly_detect_RCA) == ["data", "slo", "operation_list"]
    assert _positional(o.RCAStream.__init__) == ["self", "slo", "operation_list"]
    assert _positional(o.sweep_rank) == ["plan", "events", "precision", "iters", "exemplars", "exemplar_kinds"]
    assert "timeline" not in _params(o.rank_windows)   # rank_windows keeps its tuples


@pytest.mark.parametrize("b", [0, 513, -1, 2.5, "30", True, None])
def test_bad_buckets_raise_before_any_device_work(b):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_timeline(None, [], [], buckets=b)
    with pytest.raises(ValueError):
        o.window_timeline(None, None, None, None, [], buckets=b)
    if b is None:   # (for the keyword None means "not asked")
        return
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, timeline=b)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, timeline=b)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, timeline=b)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], timeline=b)


@pytest.mark.parametrize("what", ["", "Self", "p99", 1, None])
def test_bad_what_raises_before_any_device_work(what):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_timeline(None, [], [], what=what)
    with pytest.raises(ValueError):
        o.window_timeline(None, None, None, None, [], what=what)


def test_bad_lists_and_grids_raise_before_any_device_work():
    from microrank_amd import _lib
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_timeline(None, [], [[1]])                        # len(ops) != len(windows)
    with pytest.raises(ValueError):
        o.windows_timeline(None, [object()], [list(range(65))])    # more than 64 ops in a window
    assert o.windows_timeline(None, [], []) == []
    a3, ok = np.ones(1), np.ones(1, np.uint8)
    whole = (None, _lib.INT64_MIN, _lib.INT64_MAX, a3, ok)
    for kw in ({}, {"origin": 0}, {"width": 5}):                   # a whole-table window has no default buckets
        with pytest.raises(ValueError, match="whole-table"):
            o.windows_timeline(None, [whole], [[0]], **kw)
    win = (None, 100, 200, a3, ok)
    for kw in ({"width": 0}, {"width": -3}, {"origin": [1, 2]}, {"width": [5, 5], "origin": 0}):
        with pytest.raises(ValueError):
            o.windows_timeline(None, [win], [[0]], **kw)


ROWS = {
    # key: start [B], cnt / sum / max [B][normal, abnormal], out [side][before, after]
    -1: {"start": [1000, 1500], "cnt": [[4, 1], [0, 2]], "sum": [[2_000_000, 700_000], [0, 9_000_000]],
         "max": [[900_000, 700_000], [0, 5_000_000]], "out": [[0, 0], [0, 0]]},
    "front": {"start": [1000, 1500], "cnt": [[7, 0], [2, 3]], "sum": [[-7000, 0], [3000, 9_000_000]],
              "max": [[-500, 0], [2000, 5_000_000]], "out": [[0, 0], [0, 0]]},
    "cart": {"start": [1000, 1500], "cnt": [[0, 1], [0, 0]], "sum": [[0, 123_456], [0, 0]],
             "max": [[0, 123_456], [0, 0]], "out": [[0, 0], [1, 0]]},
    "unranked": {"start": [1000, 1500], "cnt": [[1, 1], [1, 1]], "sum": [[1, 1], [1, 1]], "max": [[1, 1], [1, 1]],
                 "out": [[0, 0], [0, 0]]},
}


def test_timeline_csv_writer(tmp_path, monkeypatch):
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    # result.csv's order is by score: cart (0.9) before front (0.5); `gone` has no rows
    o._write_timeline(["front", "gone", "cart"], [0.5, 0.7, 0.9], ROWS)
    rows = list(csv.reader(open("timeline.csv")))
    assert rows[0] == ["result", "rank", "bucket", "start", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                       "max_abnormal", "max_normal"]

    def ms(v):   # latency.csv's conversion: the SLO's unit and rounding
        return str(float(np.round(np.float64(v) / 1000.0, 4)))

    assert rows[1:] == [
        ["*", "0", "0", "1000", "1", "4", ms(700_000), ms(2_000_000 / 4), ms(700_000), ms(900_000)],
        ["*", "0", "1", "1500", "2", "0", ms(9_000_000 / 2), "0.0", ms(5_000_000), "0.0"],
        ["cart", "1", "0", "1000", "1", "0", ms(123_456), "0.0", ms(123_456), "0.0"],
        ["cart", "1", "1", "1500", "0", "0", "0.0", "0.0", "0.0", "0.0"],
        ["front", "3", "0", "1000", "0", "7", "0.0", ms(-7000 / 7), "0.0", ms(-500)],
        ["front", "3", "1", "1500", "3", "2", ms(9_000_000 / 3), ms(3000 / 2), ms(5_000_000), ms(2000)],
    ]
    assert rows[1][6:] == ["700.0", "500.0", "700.0", "900.0"] and rows[3][6] == "123.456" and rows[5][7] == "-1.0"
    assert os.listdir(tmp_path) == ["timeline.csv"]


def test_no_file_without_the_keyword(tmp_path, monkeypatch):
    """Without timeline nothing of the timeline evidence is kept or written (the driver's side of this is
    tests/test_gpu_timeline.py::test_driver_writes_timeline_csv)."""
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    o._write_result(["a", "b"], [0.1, 0.2])
    assert os.listdir(tmp_path) == ["result.csv"]
    # sweep_rank drops a stale answer of an earlier call: no "timeline" key is left for the replay
    plan = {"timeline": {0: {}}, "calls": 1, "step_n": 1, "grain": 1}
    assert o.sweep_rank(plan, []) == {} and "timeline" not in plan and "calls" not in plan
