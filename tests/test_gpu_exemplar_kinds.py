"""One exemplar per trace kind on the GPU: mr_graph_exemplars_ex with MR_EX_DISTINCT_KINDS through
DeviceGraph.exemplars_raw(..., distinct_kinds=True).

Exact checks compare with exemplar_kinds_util.distinct_top applied to the GPU's own
mr_graph_trace_rank vector (the selection reads that vector bit for bit) and the kinds of the uploaded
graph (kind_ids: pagerank.py:54-66's exact classes): traces, score bits, counts and class sizes are all
equal.  Against the oracle's vector (exemplar_util.trace_rank_ref) scores agree to 1e-9 relative (fp32
rankings 1e-4) and the kind sequence wherever the oracle separates neighbouring representatives by more
than that.

Graphs: two small general graphs with many multi-member kinds (P_rs != P_sr: members of a kind have
different scores, so a kind's best member is often not its first), a fused P_rs == P_sr graph of 600
ops / 3000 traces with 224 multi-member kinds (equal scores inside a kind), and a graph built from spans with many duplicated
call paths.  MR_EX_BLOCKS = 1 / 7 / default reach one block, a merge of ragged slices and the default cut.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import oracle as orc
from exemplar_kinds_util import distinct_top, kind_ids, kinds_in_row
from exemplar_util import rows_by_op, top_traces, trace_rank_ref
from gpu_util import general_graph, host_graph_from_oracle

pytestmark = pytest.mark.gpu

RTOL = {"fp64": 1e-9, "fp32": 1e-4}
RANKINGS = (("fp64", 25), ("fp32", 7))
MS = (1, 8, 32)
MAKE = {
    "g40": lambda: general_graph(40, 600, 5, mean_len=2),
    "g24": lambda: general_graph(24, 1500, 3, mean_len=2, multiset=0.0),
    "pf": lambda: general_graph(600, 3000, 7, mean_len=2, rs_drop=0, rs_add=0, pr_frac=None, empty_frac=0),
}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("MR_EX_BLOCKS", "MR_KIND_TEST_COLLIDE"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """g, hg, kid, class sizes, P_sr rows, the preference per anomaly flag -- shared, read-only."""
    g = MAKE[name]()
    hg = host_graph_from_oracle(g)
    kid = kind_ids(g)
    size = np.bincount(kid)[kid]
    kinds = orc.trace_kinds(g)
    np.testing.assert_array_equal(size.astype(np.float64), kinds)
    v = {a: orc.preference(g, kinds, a) for a in (False, True)}
    for a in (kid, size, *v.values()):
        a.setflags(write=False)
    return types.SimpleNamespace(g=g, hg=hg, kid=kid, size=size, rows=rows_by_op(g.sr_t, g.sr_o, g.N), v=v)


@functools.lru_cache(maxsize=None)
def r_ref(name, anomaly, K):
    c = case(name)
    r = trace_rank_ref(c.g, c.v[anomaly], K)
    r.setflags(write=False)
    return r


def _upload(hg):
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    return DeviceGraph.upload(_lib.default_context(), hg)


def _bytes(res):
    return [a.tobytes() for a in res]


def _ask(dg, ops, m, mp=None, blocks=None):
    """Every op in calls of 64 (exemplars_raw cuts them), under a block count."""
    if mp is not None:
        if blocks is None:
            mp.delenv("MR_EX_BLOCKS", raising=False)
        else:
            mp.setenv("MR_EX_BLOCKS", blocks)
    return dg.exemplars_raw(ops, m, True)


def _assert_exact(res, ops, m, r, kid, size, rows, what):
    """res against distinct_top on the GPU's own vector r: traces, score bits, counts, class sizes."""
    tr, sc, cnt, mult = res
    assert tr.shape == sc.shape == mult.shape == (len(ops), m) and cnt.shape == (len(ops),)
    assert tr.dtype == mult.dtype == cnt.dtype == np.int32 and sc.dtype == np.float64
    for i, op in enumerate(ops):
        w = f"{what} m={m} op {op} (coverage {len(rows[op])}, kinds {kinds_in_row(rows[op], kid) if len(rows[op]) else 0})"
        want = distinct_top(rows[op], r, kid, m)
        n = want.size
        assert n == min(m, kinds_in_row(rows[op], kid) if len(rows[op]) else 0), w
        assert cnt[i] == n, w
        np.testing.assert_array_equal(tr[i, :n], want, err_msg=w)
        assert sc[i, :n].tobytes() == r[want].tobytes(), w
        np.testing.assert_array_equal(mult[i, :n], size[want], err_msg=w)
        assert (tr[i, n:] == -1).all() and (sc[i, n:] == 0.0).all() and not np.signbit(sc[i, n:]).any(), w
        assert (mult[i, n:] == 0).all(), w


def _assert_oracle(res, ops, m, ref, kid, rows, rtol, what):
    """Scores against the oracle's representatives; the kind sequence where the oracle separates neighbours."""
    tr, sc, cnt, _ = res
    worst = 0.0
    for i, op in enumerate(ops):
        w = f"{what} m={m} op {op}"
        if not len(rows[op]):
            assert cnt[i] == 0, w
            continue
        reps = distinct_top(rows[op], ref, kid, len(rows[op]))   # every kind of the row, oracle order
        n = min(m, reps.size)
        assert cnt[i] == n, w
        s = ref[reps]
        np.testing.assert_allclose(sc[i, :n], s[:n], rtol=rtol, atol=0, err_msg=w)
        worst = max(worst, float(np.max(np.abs(sc[i, :n] - s[:n]) / np.maximum(s[:n], 1e-300))))
        gap_prev = np.concatenate(([np.inf], s[:-1] - s[1:]))
        gap_next = np.concatenate((s[:-1] - s[1:], [np.inf]))
        apart = np.minimum(gap_prev, gap_next)[:n] > rtol * s[:n]
        np.testing.assert_array_equal(kid[tr[i, :n]][apart], kid[reps[:n]][apart], err_msg=w)
        assert len(set(kid[tr[i, :n]].tolist())) == n and np.isin(tr[i, :n], rows[op]).all(), w
    print(f"{what} m={m}: max rel diff vs the oracle's representatives {worst:.3e}")


# ---------------------------------------------------------------------------- 1. / 2. / 3. selection
@pytest.mark.parametrize("precision,K", RANKINGS)
@pytest.mark.parametrize("name", ["g40", "g24", "pf"])
def test_selection_is_exact_and_cut_independent(name, precision, K):
    c = case(name)
    ops = list(range(c.hg.N))
    dg = _upload(c.hg)
    dg.pagerank(True, iters=K, precision=precision)
    r = dg.trace_rank()
    with pytest.MonkeyPatch.context() as mp:
        for m in MS:
            got = {b: _ask(dg, ops, m, mp, b) for b in ("1", "7", None)}
            _assert_exact(got[None], ops, m, r, c.kid, c.size, c.rows, f"{name} {precision}")
            for b in ("1", "7"):
                assert _bytes(got[b]) == _bytes(got[None]), (name, m, b)
            assert _bytes(_ask(dg, ops, m, mp, None)) == _bytes(got[None]), "two runs differ"
            _assert_oracle(got[None], ops, m, r_ref(name, True, K), c.kid, c.rows, RTOL[precision], f"{name} {precision}")
    # entry 0 is the plain entry's entry 0, bit for bit; a row of singleton kinds is the plain row
    tr, sc, cnt, mult = dg.exemplars_raw(ops, 8, True)
    ptr_, psc, pcnt = dg.exemplars_raw(ops, 8)
    has = pcnt > 0
    assert (cnt > 0).tolist() == has.tolist()
    assert tr[has, 0].tobytes() == ptr_[has, 0].tobytes() and sc[has, 0].tobytes() == psc[has, 0].tobytes()
    single = [o for o in ops if len(c.rows[o]) and (c.size[c.rows[o]] == 1).all()]
    for o in single:
        assert (tr[o].tobytes(), sc[o].tobytes(), cnt[o]) == (ptr_[o].tobytes(), psc[o].tobytes(), pcnt[o]), o
        assert (mult[o, :cnt[o]] == 1).all()
    changed = sum(tr[o].tobytes() != ptr_[o].tobytes() for o in ops)
    print(f"{name} {precision}: ops whose top-8 changes {changed} of {len(ops)}, rows of singletons {len(single)}")
    if name == "g40":   # (test_exemplar_kinds_surface: the option changes lists on this graph)
        assert changed >= 1
    dg.close()


def test_equal_scores_inside_a_kind():
    """P_rs == P_sr: 224 kinds with more than one member, whose members have the same score up to the
    last bits -- a kind's place is decided by identity, its representative by the index order."""
    c = case("pf")
    assert c.hg.rs_off is None and c.hg.pr_trace is None and int((np.bincount(c.kid) > 1).sum()) == 224
    dg = _upload(c.hg)
    dg.pagerank(True)
    r = dg.trace_rank()
    hi, lo = np.zeros(c.kid.max() + 1), np.full(c.kid.max() + 1, np.inf)
    np.maximum.at(hi, c.kid, r)
    np.minimum.at(lo, c.kid, r)
    assert ((hi - lo) <= 1e-12 * hi).all()
    dg.close()


# ---------------------------------------------------------------------------- 4. edge cases
def test_k0_duplicates_uncovered_and_the_limits():
    c = case("g40")
    dg = _upload(c.hg)
    dg.pagerank(False, iters=0)
    r = dg.trace_rank()
    assert (r == 1.0 / (c.hg.N + c.hg.T)).all()
    ops = list(range(c.hg.N))
    res = dg.exemplars_raw(ops, 32, True)
    _assert_exact(res, ops, 32, r, c.kid, c.size, c.rows, "K=0")
    for o in ops:   # every kind by its smallest index, the kinds in index order
        first = np.sort([c.rows[o][c.kid[c.rows[o]] == k].min() for k in np.unique(c.kid[c.rows[o]])])[:32]
        np.testing.assert_array_equal(res[0][o, :res[2][o]], first)
    dg.pagerank(True)
    r = dg.trace_rank()
    cov = np.array([len(x) for x in c.rows])
    top = int(np.argmax(cov))
    twice = [top, 3, top]
    res = dg.exemplars_raw(twice, 8, True)
    _assert_exact(res, twice, 8, r, c.kid, c.size, c.rows, "an op asked twice")
    assert res[0][0].tobytes() == res[0][2].tobytes() and res[3][0].tobytes() == res[3][2].tobytes()
    full = ([top] + [o for o in ops if o != top] * 2)[:64]   # n_ops = 64 with m = 32
    assert len(full) == 64
    with pytest.MonkeyPatch.context() as mp:
        for b in ("1", "7", None):
            _assert_exact(_ask(dg, full, 32, mp, b), full, 32, r, c.kid, c.size, c.rows, f"64 x 32 blocks={b}")
    dg.close()


def test_an_op_no_trace_holds():
    g = general_graph(300, 200, 3)   # (test_exemplar_surface's graph: ops outside every trace)
    hg = host_graph_from_oracle(g)
    rows = rows_by_op(g.sr_t, g.sr_o, g.N)
    none = [o for o in range(g.N) if not len(rows[o])]
    assert none
    kid = kind_ids(g)
    dg = _upload(hg)
    dg.pagerank(True)
    ops = [none[0], int(np.argmax([len(x) for x in rows])), none[-1]]
    res = dg.exemplars_raw(ops, 4, True)
    _assert_exact(res, ops, 4, dg.trace_rank(), kid, np.bincount(kid)[kid], rows, "uncovered")
    assert res[2].tolist()[0] == 0 == res[2].tolist()[2]
    assert (res[0][0] == -1).all() and (res[1][0] == 0.0).all() and (res[3][0] == 0).all()
    dg.close()


@functools.lru_cache(maxsize=None)
def span_case():
    """2000 traces over 12 ops with few distinct call paths (window_exemplar_cases' `ties` table), the
    graph of every trace: (span table, oracle graph, kid by graph trace index)."""
    from microrank_amd import synth

    st = synth.gen_spans(synth.make_topology(12, 3), 2000, 11, branch=1.2, p_max=0.5)
    g = orc.span_graph(st.trace, st.podop, st.span, st.parent, np.ones(st.n_traces, bool)).as_graph()
    kid = kind_ids(g)
    assert np.unique(kid).size * 4 < g.T   # many duplicated kinds
    return st, g, kid


def test_a_graph_built_from_spans():
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans, PagerankGraph

    st, g, kid = span_case()
    ctx = _lib.default_context()
    dev = DeviceSpans(ctx, st)
    pg = PagerankGraph(ctx, st, dev, np.ones(st.n_traces, bool))
    dg = pg.device_graph()
    # the oracle graph's kinds and rows in the device graph's node / trace order (both name their codes)
    t_of = {int(c): i for i, c in enumerate(g.traces)}
    o_of = {int(c): i for i, c in enumerate(g.nodes)}
    tmap = np.array([t_of[int(c)] for c in pg.trace_code])     # device trace index -> oracle trace index
    back = np.empty_like(tmap)
    back[tmap] = np.arange(tmap.size)
    assert sorted(tmap.tolist()) == list(range(g.T)) and len(pg.node_podop) == g.N
    kid = kid[tmap]
    orows = rows_by_op(g.sr_t, g.sr_o, g.N)
    rows = [np.sort(back[orows[o_of[int(c)]]]) for c in pg.node_podop]
    size = np.bincount(kid)[kid]
    ops = list(range(g.N))
    for precision, K in RANKINGS:
        dg.pagerank(False, iters=K, precision=precision)
        r = dg.trace_rank()
        kinds_dev = dg.fetch(kinds=True)[2]
        np.testing.assert_array_equal(kinds_dev, size.astype(np.float64))
        with pytest.MonkeyPatch.context() as mp:
            for m in (8, 32):
                got = {b: _ask(dg, ops, m, mp, b) for b in ("1", "7", None)}
                _assert_exact(got[None], ops, m, r, kid, size, rows, f"spans {precision}")
                assert _bytes(got["1"]) == _bytes(got[None]) == _bytes(got["7"])
    dg.close()
    dev.close()


@pytest.mark.parametrize("name", ["ragged_tile", "su_global_rs_is_sr", "wide"])
def test_other_forms_of_the_graph(name):
    """test_gpu_exemplars' graphs that reach the other forms the selection reads: the tile path with
    P_rs given apart and traces without ops (one kind of their own), relabelled ops with su in global
    memory, and the smallest wide graph (N > 16384)."""
    from test_gpu_exemplars import case as plain_case, rows as plain_rows

    c = plain_case(name)
    kid = kind_ids(c.g)
    size = np.bincount(kid)[kid]
    if hasattr(c, "kind"):
        np.testing.assert_array_equal(size.astype(np.float64), c.kind)
    rows = plain_rows(name)
    cov = np.array([len(x) for x in rows])
    ops = [int(o) for o in np.argsort(-cov, kind="stable")[:: max(1, cov.size // 60)][:64]]
    dg = _upload(c.hg)
    dg.pagerank(True)
    r = dg.trace_rank()
    before = _bytes(dg.fetch(kinds=True))
    with pytest.MonkeyPatch.context() as mp:
        for m in (8, 32):
            got = {b: _ask(dg, ops, m, mp, b) for b in ("7", None)}
            _assert_exact(got[None], ops, m, r, kid, size, rows, name)
            assert _bytes(got["7"]) == _bytes(got[None]), (name, m)
    assert _bytes(dg.fetch(kinds=True)) == before and dg.trace_rank().tobytes() == r.tobytes()
    dg.close()


# ---------------------------------------------------------------------------- 5. the kinds' retry path
@pytest.mark.parametrize("env", [{"MR_KIND_TEST_COLLIDE": "1"}, {"MR_KIND_PART_MIN": "1"},
                                 {"MR_KIND_TEST_COLLIDE": "1", "MR_KIND_PART_MIN": "1"}],
                         ids=["collide", "partitions", "collide-partitions"])
def test_kind_hash_collisions_do_not_change_the_answer(monkeypatch, env):
    """The lazy kinds under MR_KIND_TEST_COLLIDE (the first seed keeps 2 bits of every key: the exact
    verification fails and the next seed reruns) and by partition instead of the hash table
    (MR_KIND_PART_MIN, read per call): the answer is the answer without them, bit for bit."""
    monkeypatch.delenv("MR_KIND_PART_MIN", raising=False)
    c = case("g24")
    ops = list(range(c.hg.N))
    want = None
    for knobs in ({}, env):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        dg = _upload(c.hg)   # (a fresh graph: the representatives are computed at its first distinct call)
        dg.pagerank(True)
        before = _bytes(dg.fetch(kinds=True)) + [dg.trace_rank().tobytes()]
        res = dg.exemplars_raw(ops, 8, True)
        _assert_exact(res, ops, 8, dg.trace_rank(), c.kid, c.size, c.rows, f"knobs={knobs}")
        assert _bytes(dg.fetch(kinds=True)) + [dg.trace_rank().tobytes()] == before
        if want is None:
            want = _bytes(res)
        assert _bytes(res) == want
        dg.close()


# ---------------------------------------------------------------------------- 6. state preservation
@pytest.mark.parametrize("name,precision", [("g40", "fp64"), ("pf", "fp64"), ("pf", "fp32")])
def test_a_distinct_call_leaves_the_ranking_state(name, precision):
    c = case(name)
    ops = list(range(min(c.hg.N, 64)))
    dg = _upload(c.hg)
    dg.pagerank(True, precision=precision)

    def state():
        return _bytes(dg.fetch(kinds=True)) + [dg.trace_rank().tobytes()] + _bytes(dg.exemplars_raw(ops, 8))

    before = state()
    first = dg.exemplars_raw(ops, 8, True)
    assert state() == before
    assert _bytes(dg.exemplars_raw(ops, 8, True)) == _bytes(first)   # (the kept representatives)
    dg.pagerank(True, precision=precision)
    assert state() == before, "the next ranking differs"
    dg.pagerank(False, precision=precision)
    r = dg.trace_rank()
    _assert_exact(dg.exemplars_raw(ops, 8, True), ops, 8, r, c.kid, c.size, c.rows, "after another ranking")
    dg.close()


# ---------------------------------------------------------------------------- 7. arguments
def _rc(dg, ops, m, flags, mult=True, h=True):
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    ops = np.asarray(ops, np.int32)
    k = len(ops) * max(m, 1)
    tr, sc, cnt, mu = np.full(k, 7, np.int32), np.full(k, 7.0), np.full(len(ops), 7, np.int32), np.full(k, 7, np.int32)
    rc = _lib.load().mr_graph_exemplars_ex(dg.h if h else None, ptr(ops, C.c_int32), len(ops), m, flags, ptr(tr, C.c_int32),
                                           ptr(sc, C.c_double), ptr(cnt, C.c_int32), ptr(mu, C.c_int32) if mult else None)
    return rc, tr, sc, cnt, mu


def test_arguments_and_state_errors():
    from microrank_amd import _lib
    from test_gpu_general_graphs import _span_case

    DK = _lib.MR_EX_DISTINCT_KINDS
    c = _span_case()   # fused, pr_trace = operation_trace: MR_PR_KIND_COMPRESS compresses it
    dg = _upload(c.hg)
    assert _rc(dg, [0], 1, DK)[0] == _lib.MR_ERR_STATE          # no ranking yet
    dg.pagerank(True, compress_kinds=True)
    assert _rc(dg, [0], 1, DK)[0] == _lib.MR_ERR_STATE          # MR_PR_KIND_COMPRESS
    dg.pagerank(True)
    assert _rc(dg, [0], 1, DK)[0] == _lib.MR_OK
    assert _rc(dg, [0], 1, DK, mult=False)[0] == _lib.MR_OK     # out_mult may be NULL
    for flags in (2, 3, 0x80000000):
        assert _rc(dg, [0], 1, flags)[0] == _lib.MR_ERR_ARG, flags
    assert _rc(dg, [0], 1, 0)[0] == _lib.MR_ERR_ARG             # flags == 0 with out_mult
    assert _rc(dg, [0], 1, DK, h=False)[0] == _lib.MR_ERR_ARG
    assert _rc(dg, [0], 0, DK)[0] == _lib.MR_ERR_ARG and _rc(dg, [0], 33, DK)[0] == _lib.MR_ERR_ARG
    assert _rc(dg, [0] * 65, 1, DK)[0] == _lib.MR_ERR_ARG and _rc(dg, [c.hg.N], 1, DK)[0] == _lib.MR_ERR_ARG
    # flags == 0 with NULL is mr_graph_exemplars, bit for bit
    ops = list(range(c.hg.N))
    rc, tr, sc, cnt, _ = _rc(dg, ops, 8, 0, mult=False)
    ptr_, psc, pcnt = dg.exemplars_raw(ops, 8)
    assert rc == _lib.MR_OK and [tr.tobytes(), sc.tobytes(), cnt.tobytes()] == _bytes((ptr_, psc, pcnt))
    # the Python entry: triples, names where the graph has them
    r = dg.trace_rank()
    kid = kind_ids(c.g)
    rows = rows_by_op(c.g.sr_t, c.g.sr_o, c.g.N)
    res = dg.exemplars([0, 1], m=4, distinct_kinds=True)
    for o in (0, 1):
        want = distinct_top(rows[o], r, kid, 4)
        names = dg.traces
        assert res[o] == [(names[t] if names is not None else int(t), r[t], int(np.bincount(kid)[kid[t]])) for t in want]
    assert dg.exemplars([0], m=4) == {0: [(t if dg.traces is None else dg.traces[t], r[t]) for t in top_traces(rows[0], r, 4)]}
    dg.close()
