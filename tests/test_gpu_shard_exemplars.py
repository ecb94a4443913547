"""mr_graph_trace_rank_sharded and mr_graph_exemplars_sharded on the GPU: ranks that share one GPU (host
collectives over gloo) rank their cut of tests/test_dist_gloo.py's window graph (60 ops / 1500 traces /
18016 pairs) and answer for the WHOLE graph.  From the CPU oracle at K = 1 and K = 25, both preferences:
the top-8 of 59-60 of the 60 ops hold traces of at least two ranks at 2 and at 4 even shards,
neighbouring scores in every op's top-9 differ by >= 6e-6 relative (the oracle's order is unambiguous
there), and the smallest coverage is 32 (m = 32 is still a full list).  Several checks share each
spawned run."""
import ctypes as C

import numpy as np
import pytest

from exemplar_util import rows_by_op, top_traces, trace_rank_ref
from shard_evidence_util import bounds_of, expected_stop, preference, run, span_run, whole_graph, window_graph

pytestmark = pytest.mark.gpu

MR_ERR_ARG, MR_ERR_STATE = 1, 7
CASES = [(a, k) for a in (False, True) for k in (25, 1)]


def _rows():
    g = window_graph()
    return rows_by_op(g.sr_t, g.sr_o, g.N)


def _check_case(res, case, cut=None, ms=(1, 8, 32), r_rtol=1e-10):
    """One (preference, iterations) of a run: the vector, then every m's answer.  Returns the vector."""
    an, K = case
    g = window_graph()
    world = len(res)
    b = bounds_of(cut, g.T, world)
    for rank, out in enumerate(res):   # global ids: the position in the ranks' concatenation
        np.testing.assert_array_equal(out[case]["gid"], np.arange(b[rank], b[rank + 1]))
    r = np.concatenate([out[case]["r"] for out in res])
    ref = trace_rank_ref(g, preference(an), K)
    print(case, cut, "max rel |r - oracle| =", np.max(np.abs(r - ref) / np.maximum(ref, 1e-300)))
    np.testing.assert_allclose(r, ref, rtol=r_rtol, atol=0)
    assert r.max() == 1.0
    rows = _rows()
    owner = np.searchsorted(np.asarray(b[1:]), np.arange(g.T), side="right")
    mixed = 0
    for m in ms:
        tr, sc, cnt = res[0][case][m]
        for out in res[1:]:
            for x, y in zip(out[case][m], (tr, sc, cnt)):
                assert x.tobytes() == y.tobytes(), "ranks disagree"
        for o in range(g.N):
            want = top_traces(rows[o], r, m)
            n = len(want)
            assert cnt[o] == n == min(m, len(rows[o]))
            np.testing.assert_array_equal(tr[o, :n], want)
            assert sc[o, :n].tobytes() == r[want].tobytes()
            assert (tr[o, n:] == -1).all() and (sc[o, n:] == 0.0).all()
            if m == 8:   # the oracle separates these neighbours by >= 6e-6
                np.testing.assert_array_equal(tr[o, :n], top_traces(rows[o], ref, m))
                mixed += len(set(owner[want])) >= 2
    if 8 in ms and cut is None:
        assert mixed >= 1, "no answered list holds traces of two ranks"
    return r


@pytest.fixture(scope="module")
def two():
    return run(2, "exemplars", errors=True, blocks=True, python=True, converge=True)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_two_ranks(two, case):
    r = _check_case(two, case)
    np.testing.assert_allclose(r, whole_graph(*case)[2], rtol=1e-12, atol=0)
    assert min(len(x) for x in _rows()) == 32


def test_four_ranks():
    res = run(4, "exemplars")
    for case in CASES:
        r = _check_case(res, case)
        np.testing.assert_allclose(r, whole_graph(*case)[2], rtol=1e-12, atol=0)


@pytest.mark.parametrize("cut", ["uneven", "empty_last"])
def test_uneven_cuts_answer_as_the_even_one(two, cut):
    """bounds [0, 40, T]: rank 0's lists are shorter than m; empty_last: rank 1 holds no trace and sends
    empty lists.  The same ids as the even cut, the scores within the preference sums' rounding."""
    case = (True, 25)
    res = run(2, "exemplars", cut=cut, cases=[case])
    assert res[0]["T"] == (40 if cut == "uneven" else window_graph().T)
    _check_case(res, case, cut=cut)
    for m in (1, 8):
        np.testing.assert_array_equal(res[0][case][m][0], two[0][case][m][0])
        np.testing.assert_allclose(res[0][case][m][1], two[0][case][m][1], rtol=1e-10, atol=0)
        np.testing.assert_array_equal(res[0][case][m][2], two[0][case][m][2])


def test_tile_path():
    case = (True, 25)
    res = run(2, "exemplars", tile=True, cases=[case, (False, 1)])
    _check_case(res, case)
    _check_case(res, (False, 1))


def test_selection_blocks_do_not_show(two):
    for out in two:
        for x, y in zip(out["blocks1"], out["blocks_default"]):
            assert x.tobytes() == y.tobytes()
        assert out["python_same"]


def test_record_follows_sharded_converge(two):
    for out in two:
        iters, same_r, same_ex = out["converge"]
        assert iters == expected_stop(True) and same_r and same_ex


def test_errors(two):
    for out in two:
        e = out["errors"]
        assert e["before_rank"] == MR_ERR_STATE and e["before_ex"] == MR_ERR_STATE
        assert e["m33"] == MR_ERR_ARG and e["ops65"] == MR_ERR_ARG
        assert e["disagree"] == MR_ERR_ARG, "a differing m must fail on every rank"
        assert isinstance(e["after"], tuple) and (e["after"][2] == 4).all()
        assert e["old_rank"] == MR_ERR_STATE and e["old_ex"] == MR_ERR_STATE
    assert two[0]["errors"]["after"][0].tobytes() == two[1]["errors"]["after"][0].tobytes()


def test_span_built_pair_answers_in_trace_codes():
    """shard.build_graph over tests/test_gpu_shard.py's span table: gid is the trace code, and the answer
    is the single-GPU DeviceGraph.exemplars of the whole table's graph in trace codes."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.graph import DeviceGraph
    from microrank_amd.preprocess_data import DeviceSpans
    from test_gpu_shard import _span_mask, _span_table

    res = span_run()
    for out in res:
        np.testing.assert_array_equal(out["gid"], out["trace_code"])
    st = _span_table()
    mask = _span_mask(st)
    ctx = _lib.Context(0)
    dev = DeviceSpans(ctx, st)
    lib = _lib.load()
    h = _lib.P()
    ctx.check(lib.mr_graph_build(ctx.h, dev.h, ptr(mask, C.c_uint8), C.byref(h)))
    n, t, nnz, e = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    lib.mr_graph_info(h, C.byref(n), C.byref(t), C.byref(nnz), C.byref(e))
    nodes, codes = np.empty(n.value, np.int32), np.empty(t.value, np.int32)
    lib.mr_graph_nodes(h, ptr(nodes, C.c_int32), ptr(codes, C.c_int32))
    whole = DeviceGraph(ctx, h, nodes, None, n.value, t.value)
    whole.pagerank(True)
    r = whole.trace_rank()
    nq = min(n.value, 64)
    tr, sc, cnt = whole.exemplars_raw(list(range(nq)), 8)
    whole.close()
    dev.close()
    ctx.close()
    got = dict(zip(np.concatenate([o["gid"] for o in res]).tolist(), np.concatenate([o["r"] for o in res]).tolist()))
    assert sorted(got) == sorted(codes.tolist())
    np.testing.assert_allclose([got[c] for c in codes.tolist()], r, rtol=1e-10, atol=0)
    xt, xs, xc = res[0]["ex"]
    assert res[1]["ex"][0].tobytes() == xt.tobytes() and res[1]["ex"][1].tobytes() == xs.tobytes()
    np.testing.assert_array_equal(res[0]["nodes"], nodes)
    np.testing.assert_array_equal(xc, cnt)
    np.testing.assert_array_equal(xt, np.where(tr >= 0, codes[np.maximum(tr, 0)], -1))
    np.testing.assert_allclose(xs, sc, rtol=1e-10, atol=0)
