"""CPU checks of the sharded evidence surface: the header declares mr_pagerank_sharded_converge,
mr_graph_trace_rank_sharded and mr_graph_exemplars_sharded and says what they reject, the built
library exports them, the ctypes table binds them, and the shard.* entry points reject bad arguments
before the library is loaded (no device needed)."""
import inspect
import os
import re

import pytest

from conftest import REPO

ENTRIES = {
    "mr_pagerank_sharded_converge": ["ctx", "g", "anomaly", "d", "alpha", "max_iters", "phi", "precision", "flags", "tol",
                                     "check_every", "iters_done", "resid", "converged_at"],
    "mr_graph_trace_rank_sharded": ["g", "r", "gid"],
    "mr_graph_exemplars_sharded": ["g", "ops", "n_ops", "m", "out_trace", "out_score", "out_n"],
}


class _NoDevice:
    """Stands where a context or a graph would: any use of it is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the argument check touched the device object (.{name})")


@pytest.fixture
def no_library(monkeypatch):
    from microrank_amd import _lib

    def load(*a, **k):
        raise AssertionError("the argument check loaded the library")

    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares_the_entry_and_its_errors(name):
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ENTRIES[name]
    comment = raw[:raw.index("int %s(" % name)].rsplit("/*", 1)[1]
    for word in ("MR_ERR_ARG", "MR_ERR_STATE", "collective", "mr_graph_build_sharded"):
        assert word in comment, (name, word)


def test_older_entries_point_to_the_new_ones():
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    comment = raw[:raw.index("int mr_pagerank_converge")].rsplit("/*", 1)[1]
    assert "mr_graph_build_sharded" in comment and "mr_pagerank_sharded_converge" in comment
    comment = raw[:raw.index("int mr_graph_trace_rank(")].rsplit("/*", 1)[1]
    assert "mr_graph_trace_rank_sharded" in comment and "mr_graph_exemplars_sharded" in comment


def test_signature_table_and_exports():
    from microrank_amd import _lib

    C = _lib.C
    assert _lib.SIGNATURES["mr_pagerank_sharded_converge"] == (
        C.c_int, [_lib.P, _lib.P, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.c_uint32, C.c_double,
                  C.c_int, _lib.i32p, _lib.f64p, _lib.i32p])
    assert _lib.SIGNATURES["mr_graph_trace_rank_sharded"] == (C.c_int, [_lib.P, _lib.f64p, _lib.i64p])
    assert _lib.SIGNATURES["mr_graph_exemplars_sharded"] == (
        C.c_int, [_lib.P, _lib.i32p, C.c_int32, C.c_int32, _lib.i64p, _lib.f64p, _lib.i32p])
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmicrorank_hip.so not built (run __graft_entry__.build())")
    assert set(ENTRIES) <= _lib.exported_symbols()


def test_python_surface():
    from microrank_amd import shard

    sig = inspect.signature(shard.sharded_converge)
    assert [p.name for p in sig.parameters.values() if p.kind != p.KEYWORD_ONLY] == ["dg", "anomaly"]
    for name, default in (("tol", inspect.Parameter.empty), ("max_iters", 200), ("check_every", 5), ("d", 0.85),
                          ("alpha", 0.01), ("phi", 0.5), ("precision", "fp64")):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert sig.parameters[name].default == default, name
    assert list(inspect.signature(shard.sharded_trace_rank).parameters) == ["dg"]
    sig = inspect.signature(shard.sharded_exemplars)
    assert list(sig.parameters) == ["dg", "ops", "m"] and sig.parameters["m"].default == 5


def _graph():
    from microrank_amd.graph import DeviceGraph

    return DeviceGraph(_NoDevice(), None, ["a", "b"], ["t"], 2, 1)


@pytest.mark.parametrize("kw", [dict(tol=-1.0), dict(tol=float("nan")), dict(tol=None), dict(tol="1e-8"),
                                dict(tol=1e-8, max_iters=0), dict(tol=1e-8, max_iters=2.5), dict(tol=1e-8, check_every=0),
                                dict(tol=1e-8, check_every=True), dict(tol=1e-8, phi=0.0)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_sharded_converge_rejects_before_any_device_work(kw, no_library):
    from microrank_amd import shard

    with pytest.raises(ValueError):
        shard.sharded_converge(_graph(), True, **kw)


@pytest.mark.parametrize("m", [0, 33, -1, True, 2.5, "5", None], ids=repr)
def test_sharded_exemplars_reject_m(m, no_library):
    from microrank_amd import shard

    with pytest.raises(ValueError, match="m must be"):
        shard.sharded_exemplars(_graph(), ["a"], m=m)


@pytest.mark.parametrize("ops", [[], (), "a", 3, None, ["a", "zz"], ["a", 2], [-1], [True], [1.5]], ids=repr)
def test_sharded_exemplars_reject_ops(ops, no_library):
    from microrank_amd import shard

    with pytest.raises(ValueError):
        shard.sharded_exemplars(_graph(), ops)
