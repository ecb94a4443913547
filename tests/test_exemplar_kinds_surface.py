"""CPU checks of the one-exemplar-per-trace-kind surface (MR_EX_DISTINCT_KINDS): the header declares
mr_graph_exemplars_ex / mr_windows_batch_exemplars_ex, the ctypes table binds them, the Python entries
reject exemplar_kinds without exemplars before the library is loaded, and the GPU tests' inputs are
not vacuous: on their general graph the option changes lists, and a kind's best member is not always
its lowest index (the insert's replace path has something to do)."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import oracle as orc
from conftest import REPO
from exemplar_kinds_util import distinct_top, kind_ids, kinds_in_row
from exemplar_util import rows_by_op, top_traces, trace_rank_ref
from gpu_util import general_graph
from test_exemplar_surface import _NoDevice, no_library  # noqa: F401  (fixture)

BATCH_ARGS = ["ctx", "n_windows", "spans", "t0", "t1", "a3", "a3_valid", "method", "top_max", "precision", "out_podop",
              "out_score", "n_out", "edges_traversed", "n_abnormal", "n_normal", "status", "iters", "tol", "check_every",
              "iters_done", "resid", "ex_m", "ex_trace", "ex_score", "ex_n"]


def _decl(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    return [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_declares_the_entries():
    raw = open(os.path.join(REPO, "include", "microrank_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert _decl(text, "mr_graph_exemplars_ex") == ["g", "ops", "n_ops", "m", "flags", "out_trace", "out_score", "out_n",
                                                    "out_mult"]
    assert _decl(text, "mr_windows_batch_exemplars") == BATCH_ARGS
    assert _decl(text, "mr_windows_batch_exemplars_ex") == BATCH_ARGS + ["ex_flags", "ex_mult"]
    assert re.search(r"enum\s*\{\s*MR_EX_DISTINCT_KINDS\s*=\s*1u?\s*\}", text)
    for entry in ("int mr_graph_exemplars_ex", "int mr_windows_batch_exemplars_ex"):
        comment = raw[:raw.index(entry)].rsplit("/*", 1)[1]
        for word in ("pagerank.py:54-66", "MR_EX_DISTINCT_KINDS", "MR_ERR_ARG", "MR_ERR_STATE"):
            assert word in comment, (entry, word)


def test_signature_table_and_exports():
    from microrank_amd import _lib

    C = _lib.C
    assert _lib.MR_EX_DISTINCT_KINDS == 1
    assert _lib.SIGNATURES["mr_graph_exemplars_ex"] == (C.c_int, [_lib.P, _lib.i32p, C.c_int32, C.c_int32, C.c_uint32,
                                                                  _lib.i32p, _lib.f64p, _lib.i32p, _lib.i32p])
    old = _lib.SIGNATURES["mr_windows_batch_exemplars"]
    assert _lib.SIGNATURES["mr_windows_batch_exemplars_ex"] == (old[0], old[1] + [C.c_uint32, _lib.i32p])
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmicrorank_hip.so not built (run __graft_entry__.build())")
    assert {"mr_graph_exemplars_ex", "mr_windows_batch_exemplars_ex"} <= _lib.exported_symbols()


def test_python_surface():
    from microrank_amd import graph, online_rca

    for f in (graph.DeviceGraph.exemplars_raw, graph.DeviceGraph.exemplars):
        assert inspect.signature(f).parameters["distinct_kinds"].default is False
    p = inspect.signature(online_rca.window_exemplars).parameters["distinct_kinds"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for f in (online_rca.rca_window, online_rca.rank_windows, online_rca.online_anomaly_detect_RCA,
              online_rca.RCAStream.__init__):
        p = inspect.signature(f).parameters["exemplar_kinds"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, f
    assert inspect.signature(online_rca.sweep_rank).parameters["exemplar_kinds"].default is False


def test_exemplar_kinds_needs_exemplars(no_library):  # noqa: F811
    from microrank_amd import online_rca

    nd = _NoDevice()
    with pytest.raises(ValueError, match="exemplar_kinds"):
        online_rca.rca_window(nd, 0, 1, {}, ctx=nd, table=nd, dev=nd, exemplar_kinds=True)
    with pytest.raises(ValueError, match="exemplar_kinds"):
        online_rca.rank_windows(nd, [nd], exemplar_kinds=True)
    with pytest.raises(ValueError, match="exemplar_kinds"):
        online_rca.sweep_rank(nd, [("window", 0, 1, 1, True)], exemplar_kinds=True)
    with pytest.raises(ValueError, match="exemplar_kinds"):
        online_rca.online_anomaly_detect_RCA(nd, {}, [], ctx=nd, exemplar_kinds=True)
    with pytest.raises(ValueError, match="exemplar_kinds"):
        online_rca.RCAStream({}, [], ctx=nd, exemplar_kinds=True)
    with pytest.raises(ValueError, match="exemplar_kinds"):
        online_rca.rank_windows(nd, [nd], exemplars=4, exemplar_kinds="yes")
    with pytest.raises(ValueError, match="m must be"):   # (the m check still comes before any device work)
        online_rca.rank_windows(nd, [nd], exemplars=0, exemplar_kinds=True)


def test_write_exemplars_columns(tmp_path, monkeypatch):
    from microrank_amd import online_rca

    monkeypatch.chdir(tmp_path)
    online_rca._write_exemplars(["a", "b"], [1.0, 2.0], {"a": [("t1", np.float64(0.5))], "b": [("t2", np.float64(1.0))]})
    assert open("exemplars.csv").read().splitlines() == ["result,rank,trace,score", "b,1,t2,1.0", "a,1,t1,0.5"]
    online_rca._write_exemplars(["a"], [1.0], {"a": [("t1", np.float64(0.5), 7)]}, True)
    assert open("exemplars.csv").read().splitlines() == ["result,rank,trace,score,traces", "a,1,t1,0.5,7"]


def test_distinct_top_order():
    r = np.array([0.5, 1.0, 0.5, 0.0, 1.0, 0.25])
    kid = np.array([0, 1, 0, 2, 1, 3])
    assert distinct_top([5, 4, 3, 2, 1, 0], r, kid, 8).tolist() == [1, 0, 5, 3]
    assert distinct_top([5, 4, 3, 2, 1, 0], r, kid, 2).tolist() == [1, 0]
    assert distinct_top([4, 2], r, kid, 8).tolist() == [4, 2]
    assert distinct_top([], r, kid, 8).tolist() == []
    assert kinds_in_row([0, 1, 2, 4], kid) == 2


@functools.lru_cache(maxsize=None)
def _general():
    g = general_graph(40, 600, 5, mean_len=2)
    kid = kind_ids(g)
    r = trace_rank_ref(g, orc.preference(g, orc.trace_kinds(g), True), 25)
    return g, kid, r


@pytest.mark.parametrize("make", [lambda: general_graph(40, 600, 5, mean_len=2),
                                  lambda: general_graph(24, 1500, 3, mean_len=2, multiset=0.0),
                                  lambda: general_graph(600, 3000, 7, mean_len=2, rs_drop=0, rs_add=0, empty_frac=0, pr_frac=None)],
                         ids=["g40", "g24", "pf"])
def test_kind_ids_are_the_oracles_classes(make):
    g = make()
    kid = kind_ids(g)
    np.testing.assert_array_equal(np.bincount(kid)[kid].astype(np.float64), orc.trace_kinds(g))


def test_inputs_are_not_vacuous():
    g, kid, r = _general()
    rw = rows_by_op(g.sr_t, g.sr_o, g.N)
    changed = [o for o in range(g.N)
               if distinct_top(rw[o], r, kid, 8).tolist() != top_traces(rw[o], r, 8).tolist()]
    assert len(changed) >= 1, "the option changes no op's top-8 on this graph"
    # a kind whose best member is not its lowest index, among the kinds of the four most covered ops
    cov = np.array([len(x) for x in rw])
    late = set()
    for o in np.argsort(-cov, kind="stable")[:4]:
        row = rw[int(o)]
        for k in np.unique(kid[row]):
            mem = row[kid[row] == k]
            best = mem[np.lexsort((mem, -r[mem]))[0]]
            if best != mem.min():
                late.add(int(k))
    print(f"ops whose top-8 changes: {len(changed)} of {g.N}; kinds led by a later member: {len(late)}")
    assert len(late) >= 1
    # entry 0 is the plain entry 0; a row of singleton kinds is answered as the plain selection
    for o in range(g.N):
        if len(rw[o]):
            assert distinct_top(rw[o], r, kid, 8)[0] == top_traces(rw[o], r, 8)[0]
