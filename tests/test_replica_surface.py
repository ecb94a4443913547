"""CPU checks of the replica evidence's surface: the header's declaration, the library's export, the ctypes
table, the Python keywords and the replicas.csv writer (no GPU needed)."""
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
    m = re.search(r"\bint\s+mr_windows_replicas\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 23 and args[-1].startswith("int32_t* status") and args[12].startswith("int32_t* rp_pod")
    assert [a.rsplit(" ", 1)[0] for a in args[7:22]] == ["const int32_t*", "const int32_t*", "int32_t", "int32_t", "int",
                                                         "int32_t*", "int64_t*", "int64_t*", "int64_t*", "int32_t*", "int32_t*",
                                                         "int32_t*", "int32_t*", "int64_t*", "int64_t*"]
    assert [a.rsplit(" ", 1)[1] for a in args[9:23]] == ["K", "m", "what", "rp_pod", "rp_cnt", "rp_sum", "rp_max", "rp_n",
                                                         "rp_live", "rp_all", "rp_place", "rp_own", "rp_tot", "status"]
    doc = re.sub(r"[\s*]+", " ", text[text.index("replica evidence"):text.index("int mr_windows_replicas")])
    for word in ("sv(p)", "ambiguous", "code order", "mr_windows_timeline's op slots", "LIVE", "total order", "rp_place",
                 "bitwise reproducible", "MR_ERR_STATE", "tested in this order", "no fallback", "THAT RANK", "1..32", "T2"):
        assert word in doc, word


def test_library_exports_the_entry():
    from microrank_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mr_windows_replicas")


def test_signature():
    from microrank_amd import _lib
    from microrank_amd._lib import P, i32p, i64p

    vpp = C.POINTER(C.c_void_p)
    assert _lib.SIGNATURES["mr_windows_replicas"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int32, C.c_int, i32p, i64p,
                  i64p, i64p, i32p, i32p, i32p, i32p, i64p, i64p, i32p])


def _params(fn):
    return inspect.signature(fn).parameters


def _positional(fn):
    return [p.name for p in _params(fn).values() if p.kind != p.KEYWORD_ONLY]


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import online_rca as o

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank):   # with window_replicas: five
        p = _params(fn)["replicas"]
        assert p.kind == p.KEYWORD_ONLY and p.default is None, fn.__name__
    for fn in (o.windows_replicas, o.window_replicas):
        p = _params(fn)
        assert p["m"].kind == p["m"].KEYWORD_ONLY and p["m"].default == 8
        assert p["what"].kind == p["what"].KEYWORD_ONLY and p["what"].default == "self"
    assert _positional(o.windows_replicas) == _positional(o.windows_call_edges) == ["ctx", "windows", "ops"]
    assert [n for n, p in _params(o.windows_replicas).items() if p.kind == p.KEYWORD_ONLY] == ["m", "what"]
    assert _positional(o.window_replicas) == _positional(o.window_calls) == ["data", "start_time", "end_time", "slo", "ops"]
    assert [n for n, p in _params(o.window_replicas).items() if p.kind == p.KEYWORD_ONLY] == ["m", "what", "ctx", "table", "dev"]
    # the positional names of the existing entries are what they were
    assert _positional(o.rca_window) == ["data", "start_time", "end_time", "slo"]
    assert _positional(o.rank_windows) == ["ctx", "windows"]
    assert _positional(o.online_anomaly_detect_RCA) == ["data", "slo", "operation_list"]
    assert _positional(o.RCAStream.__init__) == ["self", "slo", "operation_list"]
    assert _positional(o.sweep_rank) == ["plan", "events", "precision", "iters", "exemplars", "exemplar_kinds"]
    assert "replicas" not in _params(o.rank_windows)   # rank_windows keeps its tuples


@pytest.mark.parametrize("m", [0, 33, -1, 2.5, "8", True, None])
def test_bad_m_raises_before_any_device_work(m):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_replicas(None, [], [], m=m)
    with pytest.raises(ValueError):
        o.window_replicas(None, None, None, None, [], m=m)
    if m is None:   # (for the keyword None means "not asked")
        return
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, replicas=m)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, replicas=m)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, replicas=m)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], replicas=m)


@pytest.mark.parametrize("what", ["", "Self", "p99", 1, None])
def test_bad_what_raises_before_any_device_work(what):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_replicas(None, [], [], what=what)
    with pytest.raises(ValueError):
        o.window_replicas(None, None, None, None, [], what=what)


def test_bad_lists_raise_before_any_device_work():
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_replicas(None, [], [[1]])                        # len(ops) != len(windows)
    with pytest.raises(ValueError):
        o.windows_replicas(None, [object()], [list(range(65))])    # more than 64 ops in a window
    assert o.windows_replicas(None, [], []) == []


ROWS = {
    # entries: (pod, cnt_abn, cnt_nor, sum_abn, sum_nor, max_abn, max_nor)
    "front": {"entries": [("front-b", 3, 2, 9_000_000, 3000, 5_000_000, 2000), ("front", 0, 7, 0, -7000, 0, -500)],
              "live": 2, "all": 3, "place": 1, "own": (0, 7, 0, -7000, 0, -500), "total": (3, 9, 9_000_000, -4000, 5_000_000, 2000)},
    "cart": {"entries": [("cart", 1, 0, 123_456, 0, 123_456, 0)], "live": 1, "all": 1, "place": 0,
             "own": (1, 0, 123_456, 0, 123_456, 0), "total": (1, 0, 123_456, 0, 123_456, 0)},
    "idle": {"entries": [], "live": 0, "all": 2, "place": -1, "own": (0,) * 6, "total": (0,) * 6},
    "unranked": {"entries": [("unranked", 1, 1, 1, 1, 1, 1)], "live": 1, "all": 1, "place": 0, "own": (1,) * 6, "total": (1,) * 6},
}


def test_replicas_csv_writer(tmp_path, monkeypatch):
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    # result.csv's order is by score: cart (0.9) before idle (0.8) and front (0.5); `gone` has no rows
    o._write_replicas(["front", "gone", "cart", "idle"], [0.5, 0.7, 0.9, 0.8], ROWS)
    rows = list(csv.reader(open("replicas.csv")))
    assert rows[0] == ["result", "rank", "pod", "is_result", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                       "max_abnormal", "max_normal", "live", "replicas"]

    def ms(v):   # latency.csv's conversion: the SLO's unit and rounding
        return str(float(np.round(np.float64(v) / 1000.0, 4)))

    assert rows[1:] == [
        ["cart", "1", "cart", "1", "1", "0", ms(123_456), "0.0", ms(123_456), "0.0", "1", "1"],
        ["front", "1", "front-b", "0", "3", "2", ms(9_000_000 / 3), ms(3000 / 2), ms(5_000_000), ms(2000), "2", "3"],
        ["front", "2", "front", "1", "0", "7", "0.0", ms(-7000 / 7), "0.0", ms(-500), "2", "3"],
    ]
    assert rows[1][6] == "123.456" and rows[2][6:10] == ["3000.0", "1.5", "5000.0", "2.0"] and rows[3][7] == "-1.0"
    assert os.listdir(tmp_path) == ["replicas.csv"]


def test_no_file_without_the_keyword(tmp_path, monkeypatch):
    """Without replicas nothing of the replica evidence is kept or written (the driver's side of this is
    tests/test_gpu_replicas.py::test_driver_and_stream_write_replicas_csv)."""
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    o._write_result(["a", "b"], [0.1, 0.2])
    assert os.listdir(tmp_path) == ["result.csv"]
    # sweep_rank drops a stale answer of an earlier call: no "replicas" key is left for the replay
    plan = {"replicas": {0: {}}, "timeline": 1, "step_n": 1, "grain": 1}
    assert o.sweep_rank(plan, []) == {} and "replicas" not in plan and "timeline" not in plan
    assert "/replicas.csv" in open(os.path.join(REPO, ".gitignore")).read().split()
