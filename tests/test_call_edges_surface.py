"""CPU checks of the call evidence's surface: the header's declaration, the library's export, the ctypes
table, the Python keywords and the calls.csv writer (no GPU needed)."""
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
    m = re.search(r"\bint\s+mr_windows_call_edges\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 19 and args[-1].startswith("int32_t* status") and args[17].startswith("int64_t* ce_tot")
    assert [a.split()[0] for a in args[11:18]] == ["int32_t*", "int64_t*", "int64_t*", "int64_t*", "int32_t*", "int32_t*",
                                                    "int64_t*"]
    doc = re.sub(r"[\s*]+", " ", text[text.index("call evidence"):text.index("int mr_windows_call_edges")])
    for word in ("T11", "operation_operation", "abnormal calls descending", "bitwise reproducible", "MR_ERR_STATE",
                 "no fallback", "4096"):
        assert word in doc, word


def test_library_exports_the_entry():
    from microrank_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mr_windows_call_edges")


def test_signature():
    from microrank_amd import _lib
    from microrank_amd._lib import P, i32p, i64p

    vpp = C.POINTER(C.c_void_p)
    assert _lib.SIGNATURES["mr_windows_call_edges"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int32, i32p, i64p, i64p, i64p,
                  i32p, i32p, i64p, i32p])


def _params(fn):
    return inspect.signature(fn).parameters


def _positional(fn):
    return [p.name for p in _params(fn).values() if p.kind != p.KEYWORD_ONLY]


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import online_rca as o

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank):
        p = _params(fn)["call_edges"]
        assert p.kind == p.KEYWORD_ONLY and p.default is None, fn.__name__
    for fn in (o.windows_call_edges, o.window_calls):
        p = _params(fn)["m"]
        assert p.kind == p.KEYWORD_ONLY and p.default == 8
    assert _positional(o.windows_call_edges) == ["ctx", "windows", "ops"]
    assert _positional(o.window_calls) == _positional(o.window_kinds) == ["data", "start_time", "end_time", "slo", "ops"]
    assert [n for n, p in _params(o.window_calls).items() if p.kind == p.KEYWORD_ONLY] == ["m", "ctx", "table", "dev"]
    # the positional names of the existing entries are what they were
    assert _positional(o.rca_window) == ["data", "start_time", "end_time", "slo"]
    assert _positional(o.rank_windows) == ["ctx", "windows"]
    assert _positional(o.online_anomaly_detect_RCA) == ["data", "slo", "operation_list"]
    assert _positional(o.RCAStream.__init__) == ["self", "slo", "operation_list"]
    assert _positional(o.sweep_rank) == ["plan", "events", "precision", "iters", "exemplars", "exemplar_kinds"]
    assert "call_edges" not in _params(o.rank_windows)   # rank_windows keeps its tuples


@pytest.mark.parametrize("m", [0, 33, -1, 2.5, "8", True, None])
def test_bad_m_raises_before_any_device_work(m):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_call_edges(None, [], [], m=m)
    with pytest.raises(ValueError):
        o.window_calls(None, None, None, None, [], m=m)
    if m is None:   # (for the keyword None means "not asked")
        return
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, call_edges=m)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, call_edges=m)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, call_edges=m)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], call_edges=m)


def test_bad_op_lists_raise_before_any_device_work():
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_call_edges(None, [], [[1]])                      # len(ops) != len(windows)
    with pytest.raises(ValueError):
        o.windows_call_edges(None, [object()], [list(range(65))])  # more than 64 ops in a window
    assert o.windows_call_edges(None, [], []) == []


ROWS = {
    # op: (callers, callees); a side: (entries, n_peers, (calls_abn, calls_nor)); an entry: (peer, calls_abn,
    # calls_nor, dsum_abn, dsum_nor, dmax_abn, dmax_nor)
    "front": (([], 0, (0, 0)),
              ([("cart", 3, 2, 9_000_000, 3000, 5_000_000, 2000), ("pay", 1, 0, 123_456, 0, 123_456, 0)], 5, (9, 2))),
    "cart": (([("front", 3, 2, 9_000_000, 3000, 5_000_000, 2000)], 1, (3, 2)),
             ([("db", 0, 7, 0, -7000, 0, -500)], 1, (0, 7))),
    "unranked": (([("x", 1, 1, 1, 1, 1, 1)], 1, (1, 1)), ([], 0, (0, 0))),
}


def test_calls_csv_writer(tmp_path, monkeypatch):
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    # result.csv's order is by score: cart (0.9) before front (0.5); `gone` has no rows
    o._write_calls(["front", "gone", "cart"], [0.5, 0.7, 0.9], ROWS)
    rows = list(csv.reader(open("calls.csv")))
    assert rows[0] == ["result", "rank", "direction", "peer", "calls_abnormal", "calls_normal", "mean_abnormal",
                       "mean_normal", "max_abnormal", "max_normal"]

    def ms(v):   # latency.csv's conversion: the SLO's unit and rounding
        return str(float(np.round(np.float64(v) / 1000.0, 4)))

    assert rows[1:] == [
        ["cart", "1", "caller", "front", "3", "2", ms(9_000_000 / 3), ms(3000 / 2), ms(5_000_000), ms(2000)],
        ["cart", "1", "callee", "db", "0", "7", "0.0", ms(-7000 / 7), "0.0", ms(-500)],
        ["front", "1", "callee", "cart", "3", "2", ms(9_000_000 / 3), ms(3000 / 2), ms(5_000_000), ms(2000)],
        ["front", "2", "callee", "pay", "1", "0", ms(123_456), "0.0", ms(123_456), "0.0"],
    ]
    assert rows[1][6] == "3000.0" and rows[4][6] == "123.456" and rows[2][7] == "-1.0"
    assert [float(x) for x in o._latency_ms([1500])] == [1.5]   # (the unit latency.csv uses)
    assert os.listdir(tmp_path) == ["calls.csv"]


def test_no_file_without_the_keyword(tmp_path, monkeypatch):
    """Without call_edges nothing of the call evidence is kept or written (the driver's side of this is
    tests/test_gpu_call_edges.py::test_driver_writes_calls_csv)."""
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    o._write_result(["a", "b"], [0.1, 0.2])
    assert os.listdir(tmp_path) == ["result.csv"]
    # sweep_rank drops a stale answer of an earlier call: no "calls" key is left for the replay
    plan = {"calls": {0: {}}, "latency": 1, "kinds": 2, "step_n": 1, "grain": 1}
    assert o.sweep_rank(plan, []) == {} and "calls" not in plan
