"""CPU checks of the endpoint evidence's surface: the header's declarations, the library's exports, the ctypes
table, the Python keywords -- kind_by among them -- and the endpoints.csv writer (no GPU needed)."""
import csv
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

DRIVER_KW = dict(kind_breakdown=4, kind_by="endpoint")


@pytest.fixture
def no_library(monkeypatch):
    from microrank_amd import _lib

    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))


def test_header_declares_the_entries():
    text = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+MR_EP_NONE\s+\(-2\)", code)
    m = re.search(r"\bint\s+mr_spans_entry_ops\s*\(([^;]*)\)\s*;", code)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["mr_ctx* ctx", "const mr_spans* s", "int32_t* ep"]
    m = re.search(r"\bint\s+mr_windows_endpoints\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 19
    assert [a.rsplit(" ", 1)[0] for a in args[7:]] == ["const int32_t*", "const int32_t*", "int32_t", "int32_t", "int32_t*",
                                                       "int64_t*", "int64_t*", "int64_t*", "int32_t*", "int32_t*", "int64_t*",
                                                       "int32_t*"]
    assert [a.rsplit(" ", 1)[1] for a in args[9:]] == ["K", "m", "ep_op", "ep_cnt", "ep_sum", "ep_max", "ep_n", "ep_live",
                                                       "ep_tot", "status"]
    doc = re.sub(r"[\s*]+", " ", text[text.index("endpoint evidence"):text.index("#define MR_EP_NONE")])
    for word in ("Root row", "parent[r] < 0", "Entry row", "largest duration", "smallest row position", "MR_EP_NONE (-2)",
                 "tend - tstart", "code order", "AT LEAST ONE", "LIVE", "total order", "MR_EP_NONE last", "ep_tot",
                 "MR_EP_CHUNK", "MR_EP_BLOCKS", "MR_ERR_STATE", "tested in this order", "per-trace index",
                 "trace-level times", "trace shard", "2^30", "no fallback", "1..32", "T2", "DISTINCT TRACES"):
        assert word in doc, word


def test_library_exports_the_entries():
    from microrank_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmicrorank_hip.so not built (run __graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mr_windows_endpoints") and hasattr(lib, "mr_spans_entry_ops")


def test_signatures():
    from microrank_amd import _lib
    from microrank_amd._lib import P, i32p, i64p

    vpp = C.POINTER(C.c_void_p)
    assert _lib.MR_EP_NONE == -2
    assert _lib.SIGNATURES["mr_spans_entry_ops"] == (C.c_int, [P, P, i32p])
    assert _lib.SIGNATURES["mr_windows_endpoints"] == (
        C.c_int, [P, C.c_int32, C.POINTER(P), i64p, i64p, vpp, vpp, i32p, i32p, C.c_int32, C.c_int32, i32p, i64p, i64p,
                  i64p, i32p, i32p, i64p, i32p])


def _params(fn):
    return inspect.signature(fn).parameters


def _positional(fn):
    return [p.name for p in _params(fn).values() if p.kind != p.KEYWORD_ONLY]


def test_keywords_are_keyword_only_with_defaults():
    from microrank_amd import evidence
    from microrank_amd import online_rca as o
    from microrank_amd.preprocess_data import DeviceSpans

    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank, evidence.evidence_request):
        p = _params(fn)["kind_by"]
        assert p.kind == p.KEYWORD_ONLY and p.default == "kind", fn.__name__
    for fn in (o.windows_endpoints, o.window_endpoints):
        p = _params(fn)["m"]
        assert p.kind == p.KEYWORD_ONLY and p.default == 8
    assert _positional(o.windows_endpoints) == _positional(o.windows_kind_breakdown) == ["ctx", "windows", "ops"]
    assert [n for n, p in _params(o.windows_endpoints).items() if p.kind == p.KEYWORD_ONLY] == ["m"]
    assert _positional(o.window_endpoints) == _positional(o.window_kinds) == ["data", "start_time", "end_time", "slo", "ops"]
    assert [n for n, p in _params(o.window_endpoints).items() if p.kind == p.KEYWORD_ONLY] == ["m", "ctx", "table", "dev"]
    for name in ("windows_endpoints", "window_endpoints", "_write_endpoints"):
        assert getattr(o, name) is getattr(evidence, name), name   # re-exported like the others
    assert list(_params(DeviceSpans.entry_ops)) == ["self"]
    # the positional names of the existing entries are what they were
    assert _positional(o.rca_window) == ["data", "start_time", "end_time", "slo"]
    assert _positional(o.sweep_rank) == ["plan", "events", "precision", "iters", "exemplars", "exemplar_kinds"]


@pytest.mark.parametrize("m", [0, 33, -1, 2.5, "8", True, None])
def test_bad_m_raises_before_the_library_is_loaded(m, no_library):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_endpoints(None, [], [], m=m)
    with pytest.raises(ValueError):
        o.window_endpoints(None, None, None, None, [], m=m)
    if m is None:   # (for the keyword None means "not asked": kind_by without kind_breakdown, below)
        return
    for kw in (dict(kind_breakdown=m, kind_by="endpoint"),):
        with pytest.raises(ValueError):
            o.rca_window(None, None, None, None, **kw)
        with pytest.raises(ValueError):
            o.RCAStream(None, None, ctx=object(), device_append=False, **kw)
        with pytest.raises(ValueError):
            o.online_anomaly_detect_RCA(None, None, None, **kw)
        with pytest.raises(ValueError):
            o.sweep_rank({}, [], **kw)


@pytest.mark.parametrize("kw", [dict(kind_by="endpoint"), dict(kind_breakdown=4, kind_by="endpoints"),
                                dict(kind_breakdown=4, kind_by=None), dict(kind_breakdown=4, kind_by=1),
                                dict(kind_by="op"), dict(kind_breakdown=4, kind_by="Endpoint")],
                         ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()))
def test_bad_kind_by_raises_before_the_library_is_loaded(kw, no_library):
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        evidence.evidence_request(**kw)
    with pytest.raises(ValueError):
        o.sweep_rank({}, [], **kw)
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, **kw)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, **kw)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, **kw)


def test_bad_lists_raise_before_the_library_is_loaded(no_library):
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        o.windows_endpoints(None, [], [[1]])                        # len(ops) != len(windows)
    with pytest.raises(ValueError):
        o.windows_endpoints(None, [object()], [list(range(65))])    # more than 64 ops in a window
    assert o.windows_endpoints(None, [], []) == []


def test_kind_by_through_the_request(no_library):
    from microrank_amd import evidence

    kinds = evidence.KINDS[1]
    assert kinds.keyword == "kind_breakdown"
    # "kind": the parameters are exactly what they were, and so are the forms
    for r in (evidence.evidence_request(kind_breakdown=6), evidence.evidence_request(kind_breakdown=6, kind_by="kind")):
        (k, params), = r.kinds
        assert k is kinds and dict(params) == {"m": 6}
        assert (k.key_for(params), k.batch_for(params), k.window_for(params)) == ("kinds", evidence.windows_kind_breakdown,
                                                                                  evidence.window_kinds)
        assert k.kwargs(params) == {"m": 6}
    # "endpoint": the same kind, the other grouping
    r = evidence.evidence_request(kind_breakdown=np.int64(5), kind_by="endpoint", replicas=3)
    assert [k.keyword for k, _ in r.kinds] == ["kind_breakdown", "replicas"]
    k, params = r.kinds[0]
    assert k is kinds and dict(params) == {"m": 5, "by": "endpoint"} and type(params["m"]) is int
    with pytest.raises(TypeError):
        params["by"] = "kind"                                       # the request is read-only
    assert (k.key_for(params), k.batch_for(params), k.window_for(params)) == ("endpoints", evidence.windows_endpoints,
                                                                              evidence.window_endpoints)
    assert k.kwargs(params) == {"m": 5} and k.keys == ("kinds", "endpoints")
    assert k.lead == (None,) and evidence.KINDS[0].keys == ("latency",)
    # the timeline's option still picks its forms
    tl, tparams = evidence.evidence_request(timeline=4, timeline_q=0.5).kinds[0]
    assert tl.batch_for(tparams) is evidence.windows_timeline_q and tl.key_for(tparams) == "timeline"
    assert tl.batch_for({"buckets": 4}) is evidence.windows_timeline


ROWS = {
    # entries: (endpoint, cnt_abn, cnt_nor, sum_abn, sum_nor, max_abn, max_nor)
    None: {"entries": [("POST /preserve", 3, 2, 9_000_000, 3000, 5_000_000, 2000), (None, 1, 0, 123_456, 0, 123_456, 0),
                       ("GET /stations", 0, 7, 0, 7000, 0, 1500)], "live": 3, "total": (4, 9, 9_123_456, 10_000, 5_000_000, 2000)},
    "front": {"entries": [("POST /preserve", 3, 0, 9_000_000, 0, 5_000_000, 0)], "live": 1,
              "total": (3, 0, 9_000_000, 0, 5_000_000, 0)},
    "cart": {"entries": [("GET /stations", 0, 2, 0, -4000, 0, -500)], "live": 4, "total": (0, 5, 0, 0, 0, 0)},
    "idle": {"entries": [], "live": 0, "total": (0,) * 6},
    "unranked": {"entries": [("x", 1, 1, 1, 1, 1, 1)], "live": 1, "total": (1,) * 6},
}


def test_endpoints_csv_writer(tmp_path, monkeypatch, no_library):
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    # result.csv's order is by score: cart (0.9) before idle (0.8) and front (0.5); `gone` has no rows
    o._write_endpoints(["front", "gone", "cart", "idle"], [0.5, 0.7, 0.9, 0.8], ROWS)
    rows = list(csv.reader(open("endpoints.csv")))
    assert rows[0] == ["result", "rank", "endpoint", "traces_abnormal", "traces_normal", "mean_abnormal", "mean_normal",
                       "max_abnormal", "max_normal", "live"]

    def ms(v):   # latency.csv's conversion: the SLO's unit and rounding
        return str(float(np.round(np.float64(v) / 1000.0, 4)))

    assert rows[1:] == [
        ["*", "0", "POST /preserve", "3", "2", ms(9_000_000 / 3), ms(3000 / 2), ms(5_000_000), ms(2000), "3"],
        ["*", "0", "(none)", "1", "0", ms(123_456), "0.0", ms(123_456), "0.0", "3"],
        ["*", "0", "GET /stations", "0", "7", "0.0", ms(1000), "0.0", ms(1500), "3"],
        ["cart", "1", "GET /stations", "0", "2", "0.0", ms(-2000), "0.0", ms(-500), "4"],
        ["front", "4", "POST /preserve", "3", "0", ms(3_000_000), "0.0", ms(5_000_000), "0.0", "1"],
    ]
    assert rows[1][5:9] == ["3000.0", "1.5", "5000.0", "2.0"] and rows[4][6] == "-2.0"
    assert os.listdir(tmp_path) == ["endpoints.csv"]
    assert "/endpoints.csv" in open(os.path.join(REPO, ".gitignore")).read().split()


def test_sweep_emit_writes_the_variants_file(tmp_path, monkeypatch, no_library):
    """The sweep's replay with kind_by="endpoint": the answer is read from plan["endpoints"], named through the endpoint
    row mapper and written to endpoints.csv; kinds.csv is not written, and sweep_rank drops a stale answer."""
    import contextlib
    import io
    from types import SimpleNamespace

    from microrank_amd import _lib, evidence
    from microrank_amd import online_rca as o

    monkeypatch.chdir(tmp_path)
    table = SimpleNamespace(podop_names=["front", "cart", "db"], trace_names=None)
    slot = {"entries": [(1, 2, 1, 5000, 1000, 4000, 1000), (None, 1, 0, 7000, 0, 7000, 0)], "live": 2,
            "total": (3, 1, 12000, 1000, 7000, 1000)}
    plan = {"table": table, "endpoints": {0: {None: slot, 2: dict(slot, live=5)}}, "step_n": 1, "grain": 1}
    results = {0: (np.array([2], np.int32), np.array([0.75]), 1, 1, 7, _lib.MR_OK)}
    request = evidence.evidence_request(**DRIVER_KW)
    with contextlib.redirect_stdout(io.StringIO()):
        o._sweep_emit(plan, [("window", 0, 1, 1, True)], results, request)
    assert sorted(os.listdir(tmp_path)) == ["endpoints.csv", "result.csv"]
    rows = list(csv.reader(open("endpoints.csv")))[1:]
    assert [r[:5] for r in rows] == [["*", "0", "cart", "2", "1"], ["*", "0", "(none)", "1", "0"],
                                     ["db", "1", "cart", "2", "1"], ["db", "1", "(none)", "1", "0"]]
    assert [r[-1] for r in rows] == ["2", "2", "5", "5"]
    assert o.sweep_rank(plan, []) == {} and "endpoints" not in plan
