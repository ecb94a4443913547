"""The windows of the window-batch exemplar tests and their oracle side (no GPU).

A case is a span table built like test_gpu_exemplars.span_window: synth.make_topology(n_ops, 3),
synth.gen_spans(topo, n_traces, seed, **kw), ONE constant SLO c for every service-op ([c, 0.0]) and the
window [tstart.min(), tend.max()].  c is the median over traces of (max duration / 1000 / span count)
-- about half of the traces abnormal -- or, for `one_trace`, the midpoint of that ratio's two largest
values: exactly one abnormal trace.

Oracle side: orc.detect, the graph of the detector's abnormal traces (orc.span_graph(..., sel)
.as_graph(), ranked with anomaly False, T1) and of its normal traces (anomaly True), orc.preference,
orc.power_iteration, orc.weights and orc.spectrum with the lists swapped as T1 does
(tests/test_gpu_window_iters.py::oracle_rank), exemplar_util.trace_rank_ref / rows_by_op.  Everything
returned is shared between tests and read-only.
"""
import functools
import types

import numpy as np

import oracle as orc
from exemplar_util import rows_by_op, trace_rank_ref

# name -> (ops, traces, seed, gen_spans keywords, SLO rule)
CASES = {
    "ragged": (30, 130, 9, {}, "median"),
    "one_trace": (30, 130, 9, {}, "top2"),
    "mid": (300, 1000, 7, {}, "median"),
    "ties": (12, 2000, 11, dict(branch=1.2, p_max=0.5), "median"),
    "span_times": (60, 600, 4, dict(span_times=True), "median"),
}
NAMES = tuple(CASES)
TOP_MAX = 5
K_TOP = TOP_MAX + 6
ITERS = {"fp64": 25, "fp32": 7}


@functools.lru_cache(maxsize=None)
def table(name):
    """(span table, SLO dict, c, t0, t1)."""
    from microrank_amd import synth

    n_ops, n_traces, seed, kw, rule = CASES[name]
    topo = synth.make_topology(n_ops, 3)
    st = synth.gen_spans(topo, n_traces, seed, **kw)
    mx = np.zeros(st.n_traces, np.int64)
    np.maximum.at(mx, st.trace, st.duration)
    cnt = np.bincount(st.trace, minlength=st.n_traces)
    ratio = mx[cnt > 0] / 1000.0 / cnt[cnt > 0]
    if rule == "median":
        c = float(np.median(ratio))
    else:
        top = np.sort(ratio)[-2:]
        assert top[1] > top[0]
        c = float((top[0] + top[1]) / 2)
    slo = {name_: [c, 0.0] for name_ in st.svcop_names}
    return st, slo, c, int(st.tstart.min()), int(st.tend.max())


@functools.lru_cache(maxsize=None)
def detected(name, scale=1.0):
    """(abnormal trace codes, normal trace codes) of the window under c * scale."""
    st, _, c, t0, t1 = table(name)
    res = orc.detect(st.trace, st.svcop, st.duration, st.tstart, st.tend, t0, t1,
                     {i: c * scale for i in range(st.n_svcops)})
    assert res is not None
    return tuple(res[1]), tuple(res[2])


@functools.lru_cache(maxsize=None)
def graphs(name):
    """[(g, v)]: index 0 the graph of the detector's abnormal traces (anomaly False, T1), 1 of its normal ones."""
    st = table(name)[0]
    ab, no = detected(name)
    out = []
    for lst, anomaly in ((ab, False), (no, True)):
        sel = np.zeros(st.n_traces, bool)
        sel[list(lst)] = True
        g = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel).as_graph()
        out.append((g, orc.preference(g, orc.trace_kinds(g), anomaly)))
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, K):
    """The window after K iterations: top (pod-op codes, top-list order), score, and for the graph of the
    abnormal traces r (the oracle's r_K by graph trace index), trace_codes, rows ({pod-op code: graph
    trace indices}; a top op absent from that graph has no entry)."""
    gs = graphs(name)
    ab, no = detected(name)
    res = []
    for g, v in gs:
        s = np.ones(g.N) / float(g.N + g.T) if K == 0 else orc.power_iteration(g, v, iters=K)
        res.append(orc.weights(g, s))   # [normal, anomaly]
    top, score, _ = orc.spectrum(res[1][0], res[0][0], len(no), len(ab), TOP_MAX, res[0][1], res[1][1], "dstar2")
    g, v = gs[0]
    r = trace_rank_ref(g, v, K)
    r.setflags(write=False)
    by_op = rows_by_op(g.sr_t, g.sr_o, g.N)
    rows = {int(code): by_op[i] for i, code in enumerate(g.nodes)}
    tc = np.asarray(g.traces, np.int64)
    tc.setflags(write=False)
    return types.SimpleNamespace(top=[int(c) for c in top], score=np.array(score, np.float64), r=r, trace_codes=tc,
                                 rows=rows, n_abnormal=len(ab), n_normal=len(no), N=g.N, T=g.T)


def coverage(name, K=25):
    """{top pod-op code: its coverage in the abnormal traces' graph (0: absent)}."""
    o = oracle(name, K)
    return {c: len(o.rows.get(c, ())) for c in o.top}


def span_pairs(name):
    st = table(name)[0]
    return set(zip(st.trace.tolist(), st.podop.tolist()))
