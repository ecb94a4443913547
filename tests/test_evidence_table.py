"""CPU checks of the evidence table (microrank_amd/evidence.py): its records, the one request that checks
every keyword before the library is loaded, the re-exports of online_rca, and that the drivers loop over
the table without naming a kind (no library needed)."""
import ast
import contextlib
import csv
import inspect
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

KEYWORDS = ["latency", "kind_breakdown", "call_edges", "timeline", "replicas"]
KEYS = ["latency", "kinds", "calls", "timeline", "replicas"]
REEXPORTED = ["windows_latency", "windows_kind_breakdown", "windows_call_edges", "windows_timeline", "windows_replicas",
              "op_latency", "window_kinds", "window_calls", "window_timeline", "window_replicas", "_write_latency",
              "_write_kinds", "_write_calls", "_write_timeline", "_write_replicas", "_latency_ms"]
# the surface tests' lists (tests/test_*_surface.py)
BAD_M = [0, 33, -1, 2.5, "8", True]
BAD = ([{"latency": q} for q in (1.5, -0.1, float("nan"), [], [0.5] * 17, "median")] +
       [{"latency": 0.5, "latency_what": w} for w in ("total", 1)] +
       [{k: m} for k in ("kind_breakdown", "call_edges", "replicas", "exemplars") for m in BAD_M] +
       [{"timeline": b} for b in (0, 513, -1, 2.5, "30", True)] +
       [{"exemplar_kinds": True}, {"exemplar_kinds": 1, "exemplars": 3}])


@pytest.fixture
def no_library(monkeypatch):
    from microrank_amd import _lib

    monkeypatch.setattr(_lib, "load", lambda *a, **k: pytest.fail("the library was loaded"))


def test_table_shape():
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    assert [k.keyword for k in evidence.KINDS] == KEYWORDS       # today's call order
    assert [k.key for k in evidence.KINDS] == KEYS
    assert [k.lead for k in evidence.KINDS] == [(), (None,), (), (-1,), ()]
    assert [k.batch for k in evidence.KINDS] == [o.windows_latency, o.windows_kind_breakdown, o.windows_call_edges,
                                                 o.windows_timeline, o.windows_replicas]
    assert [k.window for k in evidence.KINDS] == [o.op_latency, o.window_kinds, o.window_calls, o.window_timeline,
                                                  o.window_replicas]
    assert [k.write for k in evidence.KINDS] == [o._write_latency, o._write_kinds, o._write_calls, o._write_timeline,
                                                 o._write_replicas]
    ignored = open(os.path.join(REPO, ".gitignore")).read().split()
    for fn in (o.rca_window, o.online_anomaly_detect_RCA, o.RCAStream.__init__, o.sweep_rank, evidence.evidence_request):
        ps = inspect.signature(fn).parameters
        for k in evidence.KINDS:
            assert ps[k.keyword].kind == ps[k.keyword].KEYWORD_ONLY and ps[k.keyword].default is None, (fn.__name__, k.keyword)
    for k in evidence.KINDS:
        assert f"/{k.key}.csv" in ignored, k.key
    imports = [n for n in ast.walk(ast.parse(open(evidence.__file__).read())) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert imports and not any("online_rca" in ast.dump(n) for n in imports)   # the drivers import the table, not it them


def test_reexports_are_the_same_objects():
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    for name in REEXPORTED:
        assert getattr(o, name) is getattr(evidence, name), name
    for name in ("_write_result", "_write_exemplars", "_exemplar_rows", "_sweep_plan", "window_exemplars", "rank_windows"):
        assert callable(getattr(o, name)), name


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v!r}"[:24] for k, v in kw.items()))
def test_request_rejects_before_the_library_is_loaded(kw, no_library):
    from microrank_amd import evidence
    from microrank_amd import online_rca as o

    with pytest.raises(ValueError):
        evidence.evidence_request(**kw)
    with pytest.raises(ValueError):                      # and so does every entry that builds one
        o.sweep_rank({}, [], **kw)
    with pytest.raises(ValueError):
        o.rca_window(None, None, None, None, **kw)
    with pytest.raises(ValueError):
        o.online_anomaly_detect_RCA(None, None, None, **kw)
    with pytest.raises(ValueError):
        o.RCAStream(None, None, ctx=object(), device_append=False, **kw)


def test_request_contents(no_library):
    from microrank_amd import evidence

    nothing = evidence.evidence_request()
    assert nothing == evidence.NOTHING == (None, False, ()) and nothing.kinds == ()
    r = evidence.evidence_request(replicas=4, exemplars=3, exemplar_kinds=True, latency=(0.5, 0.99), latency_what="duration",
                                  timeline=np.int64(8), call_edges=5, kind_breakdown=6)
    assert (r.exemplars, r.exemplar_kinds) == (3, True)
    assert [k.keyword for k, _ in r.kinds] == KEYWORDS           # table order, whatever the call's
    params = [dict(p) for _, p in r.kinds]
    assert params[0]["q"].tolist() == [0.5, 0.99] and params[0]["what"] == "duration"
    assert params[1:] == [{"m": 6}, {"m": 5}, {"buckets": 8}, {"m": 4}] and type(params[3]["buckets"]) is int
    with pytest.raises(TypeError):
        r.kinds[1][1]["m"] = 7                                   # the request is read-only
    only = evidence.evidence_request(timeline=30)
    assert [k.key for k, _ in only.kinds] == ["timeline"] and only.exemplars is None
    # latency's plan value is the (q, answers) pair; every other kind's the answers
    lat, kinds = evidence.KINDS[0], evidence.KINDS[1]
    assert lat.plan_value({"q": "Q"}, {0: 1}) == ("Q", {0: 1}) and lat.answers(("Q", {0: 1})) == {0: 1}
    assert kinds.plan_value({"m": 4}, {0: 1}) == {0: 1} and kinds.answers({0: 1}) == {0: 1}


def test_window_loop_signature():
    from microrank_amd import online_rca as o

    ps = list(inspect.signature(o._window_loop).parameters.values())
    assert [p.name for p in ps[:6]] == ["data", "slo", "operation_list", "current_time", "end", "iters"]
    assert ps[5].default == 25 and all(p.kind == p.POSITIONAL_OR_KEYWORD for p in ps[:6])
    assert [p.name for p in ps[6:]] == ["evidence"] and ps[6].default is None
    assert list(inspect.signature(o._sweep_run).parameters) == ["plan", "iters", "evidence"]
    assert list(inspect.signature(o._sweep_emit).parameters) == ["plan", "events", "results", "evidence"]


def test_drivers_do_not_name_the_kinds(tmp_path, monkeypatch, no_library):
    """A sixth record, added to the table alone, is popped by sweep_rank and written by _sweep_emit."""
    from microrank_amd import _lib, evidence
    from microrank_amd import online_rca as o

    written = []
    fake = evidence.Kind("fake", "fakes", lambda v: {"m": int(v)}, (), None, None,
                         lambda table, slot: ("row", slot), lambda *a: written.append(a))
    monkeypatch.setattr(evidence, "KINDS", evidence.KINDS + (fake,))
    monkeypatch.chdir(tmp_path)
    table = SimpleNamespace(podop_names=["front", "cart", "db"], trace_names=None)
    plan = {"table": table, "fakes": {0: {2: "slot-db", 0: "slot-front"}, 9: {1: "another window's"}}, "step_n": 1, "grain": 1}
    events = [("window", 0, 1, 1, True)]
    results = {0: (np.array([2, 0], np.int32), np.array([0.25, 0.75]), 1, 1, 7, _lib.MR_OK)}
    request = evidence.Evidence(None, False, ((fake, {"m": 3}),))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        o._sweep_emit(plan, events, results, request)
    assert buf.getvalue().splitlines() == [
        "anormaly_trace 1", "total_trace 2", "", "anomaly_list 1", "normal_list 1", "total 2",
        "%-50s: %.8f" % ("db", 0.25), "%-50s: %.8f" % ("front", 0.75),
        f"{['db', 'front']} {[np.float64(0.25), np.float64(0.75)]}"]
    assert list(csv.reader(open("result.csv"))) == [["level", "result", "rank", "confidence"], ["span", "front", "1", "0.75"],
                                                    ["span", "db", "2", "0.25"]]
    assert os.listdir(tmp_path) == ["result.csv"]
    assert written == [(["db", "front"], [0.25, 0.75], {"db": ("row", "slot-db"), "front": ("row", "slot-front")})]
    # sweep_rank drops a stale answer of the fake kind as it does the others'
    assert o.sweep_rank(plan, []) == {} and "fakes" not in plan and plan["table"] is table
