"""Exemplar traces on the GPU: mr_graph_trace_rank (the trace half of a ranking, the reference's
request_ranking_vector, pagerank.py:119-127) and mr_graph_exemplars (each asked op's top traces),
through DeviceGraph.trace_rank / exemplars, trace_pagerank(trace_result=), window_exemplars and
rca_window(exemplars=).

Graphs: the general graphs of test_gpu_general_graphs (seed 3) -- the smallest that reach each form of
the iteration the trace vector is read from: T = 1; the tile path with empty traces (w_t = 0), a pr
subset and P_rs != P_sr; the fused path with the last-block finish, with relabelled ops / su in
global memory; two 600-op graphs in one batch (pf launches, closing k_fx_b); the smallest wide graph
of wide_cases.  The regime of each is asserted on the host first.

Reference for r_K: exemplar_util.trace_rank_ref, one P_rs product from the oracle's s_{K-1}
(test_exemplar_surface checks it against the two-vector iteration on the CPU).  fp64 1e-10 relative on
every entry, an exact 0 stays an exact 0; fp32 1e-4 (the project's bounds).  Selection is compared
bit for bit with numpy on the GPU's own fetched vector, and as score sequences with the oracle's
(consecutive r values of these graphs lie as close as 4e-11 relative: trace identity at a near-tie
is not a fair claim).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from exemplar_util import rows_by_op, top_traces, trace_rank_ref
from gpu_util import general_graph, host_graph_from_oracle
from test_gpu_general_graphs import FX_NMAX, _assert_regime, _case as _general_case, _span_case

pytestmark = pytest.mark.gpu

RTOL64, RTOL32 = 1e-10, 1e-4
KS = (0, 1, 2, 3, 25)   # both q buffers, all three ring slots
GENERAL = ("one_trace", "ragged_tile", "long_pairs", "fused_pr_subset", "su_global_rs_is_sr")
CASES = GENERAL + ("wide",)
FP32_CASES = ("long_pairs", "fused_pr_subset")
PF_KNOBS = dict(rs_drop=0, rs_add=0, empty_frac=0, pr_frac=None)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv("MR_EX_BLOCKS", raising=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """g (oracle graph), hg (host arrays), pref[anomaly] -- read-only, shared."""
    if name == "wide":
        import wide_cases

        c = wide_cases.case("W1")
        assert c.shape.wide and c.hg.N > FX_NMAX and not c.shape.tile_path
        return c
    if name in ("pf0", "pf1"):
        from test_gpu_general_graphs import _with_oracle

        g = general_graph(600, 3000, 3 if name == "pf0" else 4, **PF_KNOBS)
        hg = host_graph_from_oracle(g)
        # fused (P_rs == P_sr, no empty trace), pr_trace = operation_trace, more ops than the last-block finish takes
        assert hg.rs_off is None and hg.pr_trace is None and (np.diff(hg.sr_off) > 0).all() and 512 < hg.N <= FX_NMAX
        return _with_oracle(g, hg)
    c = _general_case(name)
    _assert_regime(name, c.hg)
    if name == "ragged_tile":   # empty traces, and 64 ops no trace holds
        assert (c.hg.len_t == 0).any() and int((np.bincount(c.hg.sr_ops, minlength=c.hg.N) == 0).sum()) >= 64
    if name == "fused_pr_subset":
        assert c.hg.N <= 512
    return c


@functools.lru_cache(maxsize=None)
def r_ref(name, anomaly, K):
    c = case(name)
    r = trace_rank_ref(c.g, c.ref[anomaly][0], K)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def rows(name):
    c = case(name)
    return rows_by_op(c.g.sr_t, c.g.sr_o, c.g.N)


def _upload(hg):
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    return DeviceGraph.upload(_lib.default_context(), hg)


def _assert_rank(r, ref, K, rtol, what):
    nz = ref > 0
    err = np.abs(r - ref)[nz] / ref[nz]
    print(f"{what} K={K}: max rel diff vs reference {err.max() if err.size else 0.0:.3e}, zeros {int((~nz).sum())}, "
          f"max {r.max():.17g}")
    assert r.dtype == np.float64 and r.shape == ref.shape
    assert ((r == 0) == (ref == 0)).all(), what
    np.testing.assert_allclose(r, ref, rtol=rtol, atol=0, err_msg=f"{what} K={K}")
    if K > 0:
        assert abs(r.max() - 1.0) <= rtol, what


# ---------------------------------------------------------------------------- 1. trace ranks
@pytest.mark.parametrize("anomaly", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_trace_rank_against_reference(name, anomaly):
    c = case(name)
    dg = _upload(c.hg)
    seen = {}
    for K in KS:
        dg.pagerank(anomaly, iters=K)
        r = dg.trace_rank()
        _assert_rank(r, r_ref(name, anomaly, K), K, RTOL64, f"{name} anomaly={anomaly}")
        assert dg.trace_rank().tobytes() == r.tobytes()   # (the cached vector)
        seen[K] = r
    assert (seen[0] == 1.0 / (c.hg.N + c.hg.T)).all()
    if c.hg.T > 1:   # a second ranking with another count replaced the cached vector
        assert seen[3].tobytes() != seen[25].tobytes()
    if name in ("ragged_tile", "long_pairs"):   # traces without ops: r' is their (1-d) v alone; exact zeros exist
        assert (c.hg.len_t == 0).any()
    if name == "long_pairs":
        assert (seen[25] == 0).any()
    if name in FP32_CASES:
        for K in KS:
            dg.pagerank(anomaly, iters=K, precision="fp32")
            _assert_rank(dg.trace_rank(), r_ref(name, anomaly, K), K, RTOL32, f"{name} fp32 anomaly={anomaly}")
    dg.close()


@pytest.mark.parametrize("anomaly", [False, True])
def test_trace_rank_of_a_pf_batch(anomaly):
    """Two 600-op fused graphs in one mr_pagerank_batch: pf launches (k_tr_a finishes the iteration
    before), the closing k_fx_b; flags (anomaly, not anomaly)."""
    from microrank_amd import _lib

    ctx, lib = _lib.default_context(), _lib.load()
    names, flags = ("pf0", "pf1"), (int(anomaly), int(not anomaly))
    dgs = [_upload(case(n).hg) for n in names]
    hs = (_lib.P * 2)(*[dg.h for dg in dgs])
    an = (C.c_int * 2)(*flags)
    for K in KS:
        ctx.check(lib.mr_pagerank_batch(ctx.h, hs, an, 2, 0.85, 0.01, K, _lib.MR_FP64, 0), "mr_pagerank_batch")
        for n, a, dg in zip(names, flags, dgs):
            _assert_rank(dg.trace_rank(), r_ref(n, bool(a), K), K, RTOL64, f"{n} anomaly={a} batched")
    for n, a, dg in zip(names, flags, dgs):
        _check_selection(n, dg, r_ref(n, bool(a), KS[-1]), ms=(8,))
        dg.close()


@pytest.mark.parametrize("anomaly", [False, True])
@pytest.mark.parametrize("name", ["ragged_tile", "fused_pr_subset", "su_global_rs_is_sr"])
def test_trace_rank_after_converge(name, anomaly):
    c = case(name)
    dg = _upload(c.hg)
    rep = dg.converge(anomaly, tol=1e-9)
    K = rep["iters"]
    assert rep["converged_at"] is not None and 1 <= K < 200
    r = dg.trace_rank()
    _assert_rank(r, trace_rank_ref(c.g, c.ref[anomaly][0], K), K, RTOL64, f"{name} converge anomaly={anomaly}")
    dg.pagerank(anomaly, iters=K)
    assert dg.trace_rank().tobytes() == r.tobytes(), "not the vector of a plain ranking with the reported count"
    dg.close()


# ---------------------------------------------------------------------------- 2. / 3. selection
def _requests(name, m_small=8):
    """(label, op indices) requests over the case's ops: the most covered op alone; 64 ops with the most
    covered one twice, an op with 0 < coverage < 8 and (where one exists) an op no trace holds."""
    cov = np.array([len(x) for x in rows(name)])
    top = int(np.argmax(cov))
    small = np.flatnonzero((cov > 0) & (cov < m_small))
    assert small.size, name
    zero = np.flatnonzero(cov == 0)
    mixed = [top, int(small[0])] + ([int(zero[0])] if zero.size else []) + [top]
    spread = np.argsort(-cov, kind="stable")[1:: max(1, cov.size // 80)]
    mixed += [int(o) for o in spread if int(o) != top][: 64 - len(mixed)]
    assert len(mixed) == 64
    out = [("top", [top]), ("mixed64", mixed)]
    if name == "ragged_tile":
        assert zero.size >= 64
        out.append(("zero64", [int(o) for o in zero[:64]]))
    return out


def _check_selection(name, dg, ref, ms=(1, 8, 32)):
    """exemplars against numpy on the GPU's own vector (bitwise), the same under three block counts,
    and as score sequences against the oracle's vector `ref`."""
    c = case(name)
    r = dg.trace_rank()
    cov_dev = dg.fetch()[1]
    rw = rows(name)
    np.testing.assert_array_equal(cov_dev, [len(x) for x in rw])
    with pytest.MonkeyPatch.context() as mp:
        for label, ops in _requests(name):
            for m in ms:
                got = {}
                for blocks in ("1", "7", None):
                    if blocks is None:
                        mp.delenv("MR_EX_BLOCKS", raising=False)
                    else:
                        mp.setenv("MR_EX_BLOCKS", blocks)
                    got[blocks] = dg.exemplars_raw(ops, m)
                tr, sc, cnt = got[None]
                for b in ("1", "7"):
                    assert [a.tobytes() for a in got[b]] == [tr.tobytes(), sc.tobytes(), cnt.tobytes()], (name, label, m, b)
                assert tr.shape == sc.shape == (len(ops), m) and cnt.shape == (len(ops),)
                for i, op in enumerate(ops):
                    n = min(m, len(rw[op]))
                    what = f"{name} {label} m={m} op {op} (coverage {len(rw[op])})"
                    assert cnt[i] == n == min(m, cov_dev[op]), what
                    want = top_traces(rw[op], r, m)
                    np.testing.assert_array_equal(tr[i, :n], want, err_msg=what)
                    assert sc[i, :n].tobytes() == r[want].tobytes(), what
                    assert (tr[i, n:] == -1).all() and (sc[i, n:] == 0.0).all() and not np.signbit(sc[i, n:]).any(), what
                    best = np.sort(ref[rw[op]])[::-1][:n]   # the oracle's n largest of the row
                    assert ((sc[i, :n] == 0) == (best == 0)).all(), what
                    np.testing.assert_allclose(sc[i, :n], best, rtol=RTOL64, atol=0, err_msg=what)
    assert c.hg.T == r.size


@pytest.mark.parametrize("name", CASES)
def test_selection_is_exact(name):
    c = case(name)
    if name == "one_trace":
        assert c.hg.T == 1     # MR_EX_BLOCKS=7: six empty slices
    if name == "ragged_tile":
        assert c.hg.T % 7      # ... and ragged ones
    dg = _upload(c.hg)
    for anomaly in (True, False):
        dg.pagerank(anomaly)
        _check_selection(name, dg, r_ref(name, anomaly, 25))
    dg.close()


def test_exemplars_by_name_and_duplicates():
    c = case("ragged_tile")
    dg = _upload(c.hg)
    dg.pagerank(True)
    r, rw = dg.trace_rank(), rows("ragged_tile")
    cov = np.array([len(x) for x in rw])
    top, none = int(np.argmax(cov)), int(np.flatnonzero(cov == 0)[0])
    res = dg.exemplars([c.hg.nodes[top], none, top], m=4)
    assert list(res) == [c.hg.nodes[top], none, top]
    want = [(c.hg.traces[t], r[t]) for t in top_traces(rw[top], r, 4)]
    assert res[c.hg.nodes[top]] == want == res[top] and res[none] == []
    assert all(isinstance(s, np.float64) for _, s in want)
    assert len(dg.exemplars(list(range(100)), m=2)) == 100   # (more than one call's 64 ops)
    dg.close()


# ---------------------------------------------------------------------------- 4. state and arguments
def _rc(dg, ops, m, n_ops=None, null=None):
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    ops = np.asarray(ops, np.int32)
    n = len(ops) if n_ops is None else n_ops
    k = max(n, 1) * max(m, 1)
    tr, sc, cnt = np.empty(k, np.int32), np.empty(k, np.float64), np.empty(max(n, 1), np.int32)
    a = dict(ops=ptr(ops, C.c_int32), tr=ptr(tr, C.c_int32), sc=ptr(sc, C.c_double), cnt=ptr(cnt, C.c_int32))
    if null:
        a[null] = None
    return _lib.load().mr_graph_exemplars(dg.h, a["ops"], n, m, a["tr"], a["sc"], a["cnt"])


def test_state_and_argument_errors():
    from microrank_amd import _lib

    lib = _lib.load()
    c = _span_case()   # fused, pr_trace = operation_trace: MR_PR_KIND_COMPRESS compresses it
    dg = _upload(c.hg)
    r = np.empty(c.hg.T)
    rp = _lib.ptr(r, C.c_double)
    assert _rc(dg, [0], 1) == _lib.MR_ERR_STATE and lib.mr_graph_trace_rank(dg.h, rp) == _lib.MR_ERR_STATE
    with pytest.raises(_lib.MRError, match="no ranking"):
        dg.trace_rank()
    dg.pagerank(True, compress_kinds=True)
    assert _rc(dg, [0], 1) == _lib.MR_ERR_STATE and lib.mr_graph_trace_rank(dg.h, rp) == _lib.MR_ERR_STATE
    with pytest.raises(_lib.MRError, match="MR_PR_KIND_COMPRESS"):
        dg.exemplars([0])
    dg.pagerank(True)   # a plain ranking afterwards works again
    assert _rc(dg, [0], 1) == _lib.MR_OK and lib.mr_graph_trace_rank(dg.h, rp) == _lib.MR_OK
    _assert_rank(r, trace_rank_ref(c.g, c.ref[True][0], 25), 25, RTOL64, "span graph")
    N = c.hg.N
    for null in ("ops", "tr", "sc", "cnt"):
        assert _rc(dg, [0], 1, null=null) == _lib.MR_ERR_ARG, null
    assert lib.mr_graph_trace_rank(dg.h, None) == _lib.MR_ERR_ARG
    assert lib.mr_graph_trace_rank(None, rp) == _lib.MR_ERR_ARG and _lib.load().mr_graph_exemplars(
        None, None, 1, 1, None, None, None) == _lib.MR_ERR_ARG
    assert _rc(dg, [0], 1, n_ops=0) == _lib.MR_ERR_ARG and _rc(dg, [0] * 65, 1) == _lib.MR_ERR_ARG
    assert _rc(dg, [0], 0) == _lib.MR_ERR_ARG and _rc(dg, [0], 33) == _lib.MR_ERR_ARG
    assert _rc(dg, [0, -1], 1) == _lib.MR_ERR_ARG and _rc(dg, [0, N], 1) == _lib.MR_ERR_ARG
    assert _rc(dg, [N - 1] * 64, 32) == _lib.MR_OK
    with pytest.raises(ValueError):
        from microrank_amd.pagerank import trace_pagerank

        trace_pagerank({"a": []}, {"t": ["a"]}, {"a": ["t"]}, {"t": ["a"]}, False, compress_kinds=True, trace_result={})
    dg.close()


# ---------------------------------------------------------------------------- 5. windows
@functools.lru_cache(maxsize=None)
def span_window():
    """60 ops / 600 traces of spans; one SLO for every op at the median of (max duration / 1000) per
    span of a trace: about half of the traces are abnormal."""
    from microrank_amd import synth

    topo = synth.make_topology(60, 3)
    st = synth.gen_spans(topo, 600, 4)
    mx = np.zeros(st.n_traces, np.int64)
    np.maximum.at(mx, st.trace, st.duration)
    cnt = np.bincount(st.trace, minlength=st.n_traces)
    c = float(np.median(mx[cnt > 0] / 1000.0 / cnt[cnt > 0]))
    slo = {name: [c, 0.0] for name in st.svcop_names}
    t0, t1 = int(st.tstart.min()), int(st.tend.max())
    _, ab, no = orc.detect(st.trace, st.svcop, st.duration, st.tstart, st.tend, t0, t1,
                           {i: c for i in range(st.n_svcops)})
    assert len(ab) >= 50 and len(no) >= 50
    return topo, st, slo, t0, t1


@pytest.fixture(scope="module")
def win():
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    topo, st, slo, t0, t1 = span_window()
    ctx = _lib.default_context()
    dev = DeviceSpans(ctx, st)
    yield ctx, st, dev, slo, t0, t1
    dev.close()


def _detect(ctx, st, dev, slo, t0, t1):
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.anormaly_detector import slo_arrays

    a3, ok = slo_arrays(st, slo)
    state = np.zeros(st.n_traces, np.uint8)
    na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
    ctx.check(_lib.load().mr_detect(ctx.h, dev.h, t0, t1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), ptr(state, C.c_uint8),
                                    C.byref(na), C.byref(nn), C.byref(nin)), "mr_detect")
    assert na.value > 0 and nn.value > 0
    return state


@pytest.mark.parametrize("precision,iters", [("fp64", 25), ("fp32", 7)])
def test_window_exemplars(win, precision, iters):
    from microrank_amd.online_rca import rca_window, window_exemplars
    from microrank_amd.preprocess_data import PagerankGraph

    ctx, st, dev, slo, t0, t1 = win
    top = rca_window(None, t0, t1, slo, ctx=ctx, table=st, dev=dev)["top"]
    assert top
    state = _detect(ctx, st, dev, slo, t0, t1)
    # an op only normal traces hold (absent from the abnormal graph), where there is one; an unknown name
    ab_ops = set(st.podop[state[st.trace] == 2].tolist())
    only_normal = [st.podop_names[c] for c in sorted(set(st.podop.tolist()) - ab_ops)][:1]
    ops = top + only_normal + ["no-such-pod_op"]
    res = window_exemplars(None, t0, t1, slo, ops, m=4, iters=iters, precision=precision, ctx=ctx, table=st, dev=dev)
    assert list(res) == ops and res["no-such-pod_op"] == [] and all(res[o] == [] for o in only_normal)
    pairs = set(zip(st.trace.tolist(), st.podop.tolist()))
    code_of_trace = {n: i for i, n in enumerate(st.trace_names)}
    code_of_op = {n: i for i, n in enumerate(st.podop_names)}
    assert any(res[o] for o in top)
    for o in top:
        scores = [s for _, s in res[o]]
        assert scores == sorted(scores, reverse=True) and len(res[o]) <= 4
        for t, s in res[o]:
            assert state[code_of_trace[t]] == 2 and (code_of_trace[t], code_of_op[o]) in pairs, (o, t)
    # the same five calls by hand: mr_detect (above), mr_graph_build, mr_pagerank_ex, mr_graph_exemplars
    pg = PagerankGraph(ctx, st, dev, state == 2)
    g = pg.device_graph()
    g.pagerank(False, iters=iters, precision=precision)
    node_of = {int(c): i for i, c in enumerate(pg.node_podop)}
    for o in top:
        i = node_of.get(code_of_op[o])
        if i is None:
            assert res[o] == []
            continue
        tr, sc, cnt = g.exemplars_raw([i], 4)
        hand = [(st.trace_names[pg.trace_code[t]], s) for t, s in zip(tr[0, :cnt[0]], sc[0, :cnt[0]])]
        assert [(t, s.tobytes()) for t, s in res[o]] == [(t, s.tobytes()) for t, s in hand], o
    g.close()


@pytest.mark.parametrize("kw", [dict(), dict(iters=9), dict(tol=1e-6, iters=60, check_every=4), dict(precision="fp32")],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "default")
def test_rca_window_exemplars(win, kw):
    from microrank_amd.online_rca import rca_window, window_exemplars

    ctx, st, dev, slo, t0, t1 = win
    info = {}
    plain = rca_window(None, t0, t1, slo, ctx=ctx, table=st, dev=dev, info=info, **kw)
    got = rca_window(None, t0, t1, slo, ctx=ctx, table=st, dev=dev, exemplars=3, **kw)
    ex = got.pop("exemplars")
    assert repr(got) == repr(plain) and np.array(got["score"]).tobytes() == np.array(plain["score"]).tobytes()
    assert list(ex) == plain["top"] and plain["top"]
    if "tol" in kw:
        assert 1 <= info["iters"] < kw["iters"]
    direct = window_exemplars(None, t0, t1, slo, plain["top"], m=3, iters=info["iters"],
                              precision=kw.get("precision", "fp64"), ctx=ctx, table=st, dev=dev)
    assert repr(ex) == repr(direct) and any(ex.values())
    assert all(len(v) <= 3 for v in ex.values())


def test_window_exemplars_without_abnormal_traces(win):
    from microrank_amd.online_rca import rca_window, window_exemplars

    ctx, st, dev, slo, t0, t1 = win
    lax = {k: [v[0] * 1e6, 0.0] for k, v in slo.items()}   # no trace exceeds it
    op = st.podop_names[0]
    assert window_exemplars(None, t0, t1, lax, [op], ctx=ctx, table=st, dev=dev) == {}
    assert window_exemplars(None, t1 + 10**12, t1 + 2 * 10**12, slo, [op], ctx=ctx, table=st, dev=dev) == {}   # empty window
    assert rca_window(None, t0, t1, lax, ctx=ctx, table=st, dev=dev, exemplars=2)["exemplars"] == {}


@pytest.mark.parametrize("anomaly", [False, True])
def test_trace_pagerank_trace_result(anomaly):
    """The drop-in dicts (get_pagerank_graph's lazy mappings, ranked on their device graph) and plain
    dicts (uploaded): keys = the trace names in order, values = the fetched vector."""
    from microrank_amd import synth
    from microrank_amd.pagerank import trace_pagerank
    from microrank_amd.preprocess_data import get_pagerank_graph

    topo, st, slo, t0, t1 = span_window()
    df = synth.to_dataframe(st, topo)
    lst = sorted(st.trace_names)[::2]
    dicts = get_pagerank_graph(lst, df)
    res = {}
    w, num = trace_pagerank(*dicts, anomaly, trace_result=res)
    w0, num0 = trace_pagerank(*dicts, anomaly)
    assert repr((w, num)) == repr((w0, num0))   # the default leaves the call as it is
    r = dicts[0].owner.device_graph().trace_rank()
    assert list(res) == list(dicts[1].keys()) == lst
    assert all(isinstance(x, np.float64) for x in res.values())
    assert np.array(list(res.values())).tobytes() == r.tobytes()
    # plain dicts of the same graph, against the oracle
    sel = np.isin(np.arange(st.n_traces), [st.trace_names.index(t) for t in lst])
    sg = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel)
    plain = orc.span_graph_dicts(sg, st.span, st.parent, st.podop_names, st.trace_names)
    res2 = {}
    trace_pagerank(*plain, anomaly, trace_result=res2, iters=6)
    g = orc.graph_from_dicts(*plain)
    assert list(res2) == list(plain[1].keys())
    _assert_rank(np.array(list(res2.values())), trace_rank_ref(g, orc.preference(g, orc.trace_kinds(g), anomaly), 6), 6,
                 RTOL64, f"plain dicts anomaly={anomaly}")
