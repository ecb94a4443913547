"""CPU checks of the convergence surface: the header declares mr_pagerank_converge, the built
library exports it, the ctypes table binds it, and the Python entry points reject bad arguments
before the library is loaded (no device needed)."""
import inspect
import os
import re

import pytest

from conftest import REPO

DICTS = ({"a": []}, {"t": ["a"]}, {"a": ["t"]}, {"t": ["a"]})


def test_header_declares_converge_and_its_limits():
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+mr_pagerank_converge\s*\(([^;]*)\)\s*;", text)
    assert m, "mr_pagerank_converge is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "ctx", "graphs", "anomaly", "n_graphs", "d", "alpha", "max_iters", "phi", "precision", "flags", "tol",
        "check_every", "iters_done", "resid", "converged_at"]
    comment = raw[:raw.index("int mr_pagerank_converge")].rsplit("/*", 1)[1]
    for word in ("README.md:37", "pagerank.py:117", "MR_PR_KIND_COMPRESS", "mr_graph_build_sharded", "mr_windows_batch",
                 "bitwise"):
        assert word in comment, word


def test_library_exports_converge():
    from microrank_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmicrorank_hip.so not built (run __graft_entry__.build())")
    assert "mr_pagerank_converge" in _lib.exported_symbols()


def test_signature_table():
    from microrank_amd import _lib

    C = _lib.C
    res, args = _lib.SIGNATURES["mr_pagerank_converge"]
    assert res is C.c_int
    assert args == [_lib.P, C.POINTER(_lib.P), C.POINTER(C.c_int), C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                    C.c_int, C.c_uint32, C.c_double, C.c_int, _lib.i32p, _lib.f64p, _lib.i32p]


def test_python_surface():
    from microrank_amd import graph, pagerank

    sig = inspect.signature(pagerank.trace_pagerank)
    for name, default in (("tol", None), ("max_iters", None), ("check_every", 5), ("info", None)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert sig.parameters[name].default == default, name
    for fn in (graph.DeviceGraph.converge, graph.converge_batch):
        sig = inspect.signature(fn)
        for name, default in (("tol", inspect.Parameter.empty), ("max_iters", 200), ("check_every", 5), ("d", 0.85),
                              ("alpha", 0.01), ("phi", 0.5), ("precision", "fp64"), ("exact_sums", False)):
            assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, name)
            assert sig.parameters[name].default == default, (fn.__name__, name)
    assert [p.name for p in inspect.signature(graph.converge_batch).parameters.values()
            if p.kind != p.KEYWORD_ONLY] == ["ctx", "graphs", "anomaly"]


class _NoDevice:
    """Stands where a context or a graph would: any use of it is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched the device object (.{name})")


@pytest.mark.parametrize("kw", [
    dict(tol=1e-8, iters=25),
    dict(tol=1e-8, compress_kinds=True),
    dict(tol=-1.0),
    dict(tol=float("nan")),
    dict(tol="1e-8"),
    dict(tol=1e-8, max_iters=0),
    dict(tol=1e-8, max_iters=2.5),
    dict(tol=1e-8, check_every=0),
    dict(tol=1e-8, phi=0.0),
    dict(tol=1e-8, info=[]),
    dict(max_iters=50),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_trace_pagerank_rejects_before_any_device_work(kw):
    from microrank_amd.pagerank import trace_pagerank

    with pytest.raises(ValueError):
        trace_pagerank(*DICTS, False, ctx=_NoDevice(), **kw)


def test_compress_kinds_error_names_the_limit():
    from microrank_amd.pagerank import trace_pagerank

    with pytest.raises(ValueError, match="compress_kinds"):
        trace_pagerank(*DICTS, False, ctx=_NoDevice(), tol=1e-8, compress_kinds=True)


@pytest.mark.parametrize("kw", [dict(tol=-1.0), dict(tol=float("nan")), dict(tol=None), dict(tol=1e-8, max_iters=0),
                                dict(tol=1e-8, check_every=0), dict(tol=1e-8, check_every=True), dict(tol=1e-8, phi=-0.5)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_converge_rejects_before_any_device_work(kw):
    from microrank_amd.graph import DeviceGraph, converge_batch

    with pytest.raises(ValueError):
        converge_batch(_NoDevice(), [_NoDevice()], [False], **kw)
    dg = DeviceGraph(_NoDevice(), None, ["a"], ["t"], 1, 1)
    with pytest.raises(ValueError):
        dg.converge(False, **kw)


def test_converge_batch_needs_one_flag_per_graph():
    from microrank_amd.graph import converge_batch

    with pytest.raises(ValueError):
        converge_batch(_NoDevice(), [_NoDevice(), _NoDevice()], [False], tol=1e-8)
    with pytest.raises(ValueError):
        converge_batch(_NoDevice(), [], [], tol=1e-8)
