"""CPU checks of the exemplar surface: the header declares mr_graph_trace_rank / mr_graph_exemplars,
the ctypes table binds them, the Python entry points reject bad arguments before the library is
loaded (no device needed), and the GPU tests' reference for the trace vector (exemplar_util) agrees
with a plain two-vector restatement of pagerank.py:116-130."""
import inspect
import os
import re

import numpy as np
import pytest

import oracle as orc
from conftest import REPO
from exemplar_util import top_traces, trace_rank_ref, two_vector_pagerank
from gpu_util import general_graph

DICTS = ({"a": []}, {"t": ["a"]}, {"a": ["t"]}, {"t": ["a"]})


class _NoDevice:
    """Stands where a context, a table or a frame would: any use of it is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched the device object (.{name})")


@pytest.fixture
def no_library(monkeypatch):
    from microrank_amd import _lib

    def load(*a, **k):
        raise AssertionError("the argument check loaded the library")

    monkeypatch.setattr(_lib, "load", load)


def test_header_declares_the_entries():
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in (("mr_graph_trace_rank", ["g", "r"]),
                       ("mr_graph_exemplars", ["g", "ops", "n_ops", "m", "out_trace", "out_score", "out_n"])):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared"
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == want
    comment = raw[:raw.index("int mr_graph_trace_rank")].rsplit("/*", 1)[1]
    for word in ("pagerank.py:119-127", "request_ranking_vector", "MR_PR_KIND_COMPRESS", "MR_ERR_STATE", "MR_ERR_ARG",
                 "coverage", "1..64", "1..32"):
        assert word in comment, word


def test_signature_table_and_exports():
    from microrank_amd import _lib

    C = _lib.C
    assert _lib.SIGNATURES["mr_graph_trace_rank"] == (C.c_int, [_lib.P, _lib.f64p])
    assert _lib.SIGNATURES["mr_graph_exemplars"] == (C.c_int, [_lib.P, _lib.i32p, C.c_int32, C.c_int32, _lib.i32p,
                                                               _lib.f64p, _lib.i32p])
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmicrorank_hip.so not built (run __graft_entry__.build())")
    assert {"mr_graph_trace_rank", "mr_graph_exemplars"} <= _lib.exported_symbols()


def test_python_surface():
    from microrank_amd import graph, online_rca, pagerank

    assert inspect.signature(graph.DeviceGraph.exemplars).parameters["m"].default == 5
    assert list(inspect.signature(graph.DeviceGraph.trace_rank).parameters) == ["self"]
    p = inspect.signature(pagerank.trace_pagerank).parameters["trace_result"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    p = inspect.signature(online_rca.rca_window).parameters["exemplars"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = inspect.signature(online_rca.window_exemplars)
    assert [q.name for q in sig.parameters.values() if q.kind != q.KEYWORD_ONLY] == ["data", "start_time", "end_time",
                                                                                     "slo", "ops"]
    for name, default in (("m", 5), ("iters", 25), ("precision", "fp64"), ("ctx", None), ("table", None), ("dev", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert sig.parameters[name].default == default, name


BAD_M = [0, 33, -1, True, 2.5, "5", None]


def _graph():
    from microrank_amd.graph import DeviceGraph

    return DeviceGraph(_NoDevice(), None, ["a", "b"], ["t"], 2, 1)


@pytest.mark.parametrize("m", BAD_M, ids=repr)
def test_exemplars_reject_m(m, no_library):
    with pytest.raises(ValueError, match="m must be"):
        _graph().exemplars(["a"], m=m)


@pytest.mark.parametrize("ops", [[], (), "a", 3, None, ["a", "zz"], ["a", 2], [-1], [True], [1.5]], ids=repr)
def test_exemplars_reject_ops(ops, no_library):
    with pytest.raises(ValueError):
        _graph().exemplars(ops)


def test_unknown_op_error_names_it(no_library):
    with pytest.raises(ValueError, match="zz"):
        _graph().exemplars(["b", "zz"], m=3)


@pytest.mark.parametrize("kw", [dict(trace_result=[]), dict(trace_result="r"), dict(trace_result={}, compress_kinds=True)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_trace_pagerank_rejects_before_any_device_work(kw, no_library):
    from microrank_amd.pagerank import trace_pagerank

    with pytest.raises(ValueError, match="trace_result"):
        trace_pagerank(*DICTS, False, ctx=_NoDevice(), **kw)


@pytest.mark.parametrize("kw", [dict(m=0), dict(m=33), dict(m=True), dict(ops=[]), dict(ops="a_op"), dict(iters=-1),
                                dict(iters=2.5)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_window_exemplars_reject_before_any_device_work(kw, no_library):
    from microrank_amd.online_rca import window_exemplars

    kw = {"ops": ["a_op"], **kw}
    with pytest.raises(ValueError):
        window_exemplars(_NoDevice(), 0, 1, {}, kw.pop("ops"), ctx=_NoDevice(), table=_NoDevice(), dev=_NoDevice(), **kw)


@pytest.mark.parametrize("m", BAD_M[:-1], ids=repr)
def test_rca_window_rejects_exemplars(m, no_library):
    from microrank_amd.online_rca import rca_window

    with pytest.raises(ValueError, match="m must be"):
        rca_window(_NoDevice(), 0, 1, {}, ctx=_NoDevice(), table=_NoDevice(), dev=_NoDevice(), exemplars=m)


@pytest.mark.parametrize("anomaly", [False, True])
def test_reference_helper_against_two_vector_restatement(anomaly):
    """trace_rank_ref (one P_rs product from the oracle's s_{K-1}) against both vectors carried through
    pagerank.py:121-127, on a general graph (P_rs != P_sr, empty traces, a pr subset): 1e-13 relative."""
    g = general_graph(300, 200, 3)
    v = orc.preference(g, orc.trace_kinds(g), anomaly)
    np.testing.assert_array_equal(trace_rank_ref(g, v, 0), np.full(g.T, 1.0 / (g.N + g.T)))
    for K in (1, 2, 25):
        s, r = two_vector_pagerank(g, v, K)
        ref = trace_rank_ref(g, v, K)
        assert ref.max() == 1.0 and ((ref == 0) == (r == 0)).all()
        np.testing.assert_allclose(ref, r, rtol=1e-13, atol=0, err_msg=f"K={K}")
        np.testing.assert_allclose(orc.power_iteration(g, v, iters=K), s, rtol=1e-13, atol=0, err_msg=f"s K={K}")


def test_top_traces_order():
    r = np.array([0.5, 1.0, 0.5, 0.0, 1.0])
    assert top_traces([4, 3, 2, 1, 0], r, 3).tolist() == [1, 4, 0]
    assert top_traces([3, 2], r, 8).tolist() == [2, 3]
    assert top_traces([], r, 8).tolist() == []
