"""Deterministic graphs and windows for the wide-graph batch tests (tests/test_gpu_wide_batches.py),
their shape facts, and their expected results from the numpy oracle (each computed once per session).

A graph with N > FX_NMAX ops ranks on the wide fused path: its WIDE_NA most covered ops stay in
k_tr_a's LDS walk, the other ("cold") entries run through k_cold_trace / k_cold_ops, one cold range
per WIDE_RW_MAX cold ops.  A narrow fused graph keeps every op's su in LDS up to SU_LDS_NMAX ops
((N + 64) * 16 B <= 160 KB - 512 B); above it the launch leaves the su-in-LDS mode.  These constants
mirror microrank_amd/csrc/mr_pr_internal.h, mr_pr_prepare.hip and mr_pr_walk.h (WV_LDS_MAX); ``shape`` computes
from the host arrays what the wide set-up makes of a graph, and tests/test_wide_cases.py asserts
the facts each case stands for, so a generator change cannot quietly turn a case narrow.

Graph cases (``case(name)``: g, hg, kind, ref[anomaly] = (preference, weights, coverage), shape):
  W1  20k ops / 6k traces, flat popularity (zipf 0.5): one cold range, >= 10000 cold entries;
  W2  30k ops / 8k traces (zipf 0.3) + 500 traces of ops >= 20000 + 64 traces of 60 ops: two cold
      ranges, traces without a hot op, tiles past the short-tile tiers;
  N1  2k ops: narrow, su in LDS;
  N2  12k ops: narrow fused, su no longer in LDS;
  TP  the 300-op general graph with P_rs != P_sr of test_gpu_general_graphs: the tile path;
  WK  W1 with every trace repeated 1, 2, 3, 1, .. times: kind compression removes real work.
Window cases (``window(name)``): WS (both span graphs wide) and WS-mixed (a higher SLO: the graph of
the detector's abnormal traces is narrow with su out of LDS, the other one wide).
"""
import functools
import types

import numpy as np

import oracle as orc
from test_gpu_general_graphs import _case as _general_case, _regime, _with_oracle
from test_gpu_pagerank import _oracle_graph_from_host, _with_cold_traces, _with_long_traces

FX_NMAX, WIDE_NA, WIDE_RW_MAX = 16384, 10000, 19456
SU_LDS_NMAX = (160 * 1024 - 512) // 16 - 64   # 10144: the largest N with every su in k_tr_a's LDS
WAVE, SHORT_CHUNKS, SHORT_COLD = 64, 5, 4     # a wave tile; ids per lane the short-tile walk takes: 4 * 5 hot, 4 cold

GRAPHS = ("W1", "W2", "N1", "N2", "TP", "WK")
WINDOWS = ("WS", "WS-mixed")
WS_OPS = 24_000
# WS-mixed's SLO = this times WS's.  Found on the CPU (detector rule + distinct ops of each side):
# factor 1.2 -> 17668 ops on the abnormal side, 1.25 -> 15253, 1.3 -> 13485, 1.35 -> 11420, 1.4 -> 9469;
# the other side keeps > 23900 ops throughout.  A constant SLO gives the split, no per-op a3 needed.
WS_MIXED_SLO_FACTOR = 1.3


def _rows_repeated(hg, counts):
    """hg with trace t repeated counts[t] times (the copies adjacent): len_o recomputed."""
    from microrank_amd.graph import HostGraph

    ln = np.diff(hg.sr_off)
    rep = np.repeat(np.arange(hg.T), counts)
    start = np.repeat(hg.sr_off[:-1][rep], ln[rep])
    within = np.arange(int(ln[rep].sum())) - np.repeat(np.cumsum(ln[rep]) - ln[rep], ln[rep])
    sr_ops = hg.sr_ops[start + within]
    sr_off = np.zeros(rep.size + 1, np.int64)
    np.cumsum(ln[rep], out=sr_off[1:])
    len_t = hg.len_t[rep]
    # entries per op: one more for every added copy of a trace that holds the op
    len_o = hg.len_o + np.bincount(sr_ops, minlength=hg.N) - np.bincount(hg.sr_ops, minlength=hg.N)
    return HostGraph(range(hg.N), range(rep.size), sr_off, sr_ops, None, None, len_t, len_o.astype(np.int32),
                     hg.ss_off, hg.ss_par, hg.nchild, None, None)


@functools.lru_cache(maxsize=None)
def host_graph(name):
    from microrank_amd import synth

    if name == "W1":
        return synth.big_graph(20_000, 6_000, seed=3, zipf_s=0.5)
    if name == "W2":
        hg = synth.big_graph(30_000, 8_000, seed=4, zipf_s=0.3)
        return _with_long_traces(_with_cold_traces(hg, 500, 20_000, seed=41), 64, 60, seed=42)
    if name == "N1":
        return synth.big_graph(2_000, 5_000, seed=5)
    if name == "N2":
        return synth.big_graph(12_000, 5_000, seed=6, zipf_s=0.5)
    if name == "TP":
        return _general_case("long_pairs").hg
    if name == "WK":
        w1 = host_graph("W1")
        return _rows_repeated(w1, np.arange(w1.T) % 3 + 1)
    raise KeyError(name)


def shape(hg):
    """What the set-up makes of a fused graph's arrays: hot ops = the WIDE_NA most covered (ties: the
    lower op first), cold entries = the others', cold ranges, traces without a hot op, the longest
    trace, tiles the short-tile walk leaves to k_cold_trace."""
    N, T = hg.N, hg.T
    cov = np.bincount(hg.sr_ops, minlength=N)
    hot = np.zeros(N, bool)
    hot[np.argsort(-cov, kind="stable")[:WIDE_NA]] = True
    t_of = np.repeat(np.arange(T), np.diff(hg.sr_off))
    n_hot_t = np.bincount(t_of, weights=hot[hg.sr_ops], minlength=T).astype(np.int64)
    n_cold_t = np.diff(hg.sr_off) - n_hot_t
    wide = N > FX_NMAX
    return types.SimpleNamespace(
        N=N, T=T, wide=wide, covered=int((cov > 0).sum()),
        cold_entries=int(n_cold_t.sum()) if wide else 0,
        cold_ranges=-(-(N - WIDE_NA) // WIDE_RW_MAX) if wide else 0,
        traces_without_hot=int((n_hot_t == 0).sum()) if wide else 0,
        max_trace=int(np.diff(hg.sr_off).max()),
        past_short_hot=int((n_hot_t > 4 * SHORT_CHUNKS).sum()) if wide else 0,
        past_short_cold=int((n_cold_t > SHORT_COLD).sum()) if wide else 0,
        su_in_lds=(not wide) and N <= SU_LDS_NMAX,
        tile_path=_regime(hg).tile_path)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's graph, host arrays, kinds, ref[anomaly] = (preference, weights, coverage) -- read-only."""
    if name == "TP":
        c = _general_case("long_pairs")
    else:
        hg = host_graph(name)
        c = _with_oracle(_oracle_graph_from_host(hg), hg)
    c.shape = shape(c.hg)
    return c


@functools.lru_cache(maxsize=None)
def history(name, anomaly, K, precision="fp64"):
    """resid[k - 1] = max|s_k - s_{k-1}| of the oracle's max-normalised iterates, k = 1..K."""
    from test_gpu_pagerank_converge import oracle_history

    return oracle_history(case(name).g, anomaly, K, precision)


@functools.lru_cache(maxsize=None)
def weights_after(name, anomaly, K):
    c = case(name)
    w, _ = orc.weights(c.g, orc.power_iteration(c.g, c.ref[anomaly][0], iters=K))
    w = np.array(list(w.values()))
    w.setflags(write=False)
    return w


# mr_pagerank_converge over this batch: the fixed count of its tol = 0 run, and a tolerance W1 reaches
# at its 4th iteration, N1 at its 4th, W2 at its 5th -- with a check every 3 iterations the call
# stops at the second check, K = 6 (converge_stop asserts the margins on the oracle's histories)
CONVERGE_BATCH = (("W1", False), ("N1", True), ("W2", True))
CONVERGE_FIXED, CONVERGE_TOL, CONVERGE_EVERY, CONVERGE_MAX = 7, 1e-3, 3, 12


@functools.lru_cache(maxsize=None)
def converge_stop():
    """(K, [converged_at per graph]) the oracle's histories give for CONVERGE_TOL: K the first check
    (every CONVERGE_EVERY iterations) where every graph's residual is <= tol.  The residuals are
    parity-bounded to 2e-10 absolute; no residual up to K may sit within 1 % of tol, every graph is
    1.5x below it at K and some graph 1.5x above it at the check before."""
    hs = [history(n, a, CONVERGE_MAX) for n, a in CONVERGE_BATCH]
    K = next(k for k in range(CONVERGE_EVERY, CONVERGE_MAX + 1, CONVERGE_EVERY)
             if all(h[k - 1] <= CONVERGE_TOL for h in hs))
    assert CONVERGE_EVERY < K < CONVERGE_MAX
    assert all(abs(h[:K] / CONVERGE_TOL - 1.0).min() > 0.01 for h in hs)
    assert all(h[K - 1] < CONVERGE_TOL / 1.5 for h in hs)
    assert any(h[K - CONVERGE_EVERY - 1] > 1.5 * CONVERGE_TOL for h in hs)
    return K, [int(np.argmax(h <= CONVERGE_TOL)) + 1 for h in hs]


# ---------------------------------------------------------------------------- windows
@functools.lru_cache(maxsize=None)
def ws_table():
    """24k ops / 16k traces of spans (5 % broken traces, 1 % duplicated root spanIDs), the non-root
    spans' ops spread over the op space as in test_wide_span_graph_with_broken_traces_against_oracle."""
    from microrank_amd import synth

    st = synth.big_spans(WS_OPS, 16_000, seed=31, dup_frac=0.01, broken_frac=0.05)
    op = st.podop.astype(np.int64)
    st.podop = st.svcop = np.where(st.parent < 0, op, (op + (st.trace.astype(np.int64) % 997) * 61) % WS_OPS
                                   ).astype(np.int32)
    return st


def _per_trace(st):
    """(max duration / 1000, span count) per trace code (every trace of the table has spans)."""
    n = st.n_traces
    mx = np.zeros(n, np.int64)
    np.maximum.at(mx, st.trace, st.duration)
    return mx / 1000.0, np.bincount(st.trace, minlength=n)


@functools.lru_cache(maxsize=None)
def ws_slo_base():
    """c: the median over traces of (max duration / 1000) / span count -- with a3[op] = c for every
    op a trace is abnormal when its own ratio exceeds c: about half of them."""
    real, cnt = _per_trace(ws_table())
    return float(np.median(real[cnt > 0] / cnt[cnt > 0]))


@functools.lru_cache(maxsize=None)
def window(name):
    """(span table, t0, t1, a3, ok) of a window case."""
    st = ws_table()
    c = ws_slo_base() * {"WS": 1.0, "WS-mixed": WS_MIXED_SLO_FACTOR}[name]
    a3 = np.full(st.n_svcops, c, np.float64)
    ok = np.ones(st.n_svcops, np.uint8)
    a3.setflags(write=False)
    ok.setflags(write=False)
    return st, int(st.tstart.min()), int(st.tend.max()), a3, ok


@functools.lru_cache(maxsize=None)
def window_graphs(name):
    """The detector's lists and the window's two oracle graphs: (n_abnormal, n_normal, [graph of the
    abnormal traces (ranked as normal, T1), graph of the normal traces (ranked as anomaly)])."""
    st, t0, t1, a3, ok = window(name)
    a3map = {i: float(a3[i]) for i in range(len(a3)) if ok[i]}
    _, ab, no = orc.detect(st.trace, st.svcop, st.duration, st.tstart, st.tend, t0, t1, a3map)
    gs = []
    for lst in (ab, no):
        sel = np.zeros(st.n_traces, bool)
        sel[lst] = True
        gs.append(orc.span_graph(st.trace, st.podop, st.span, st.parent, sel).as_graph())
    return len(ab), len(no), gs


@functools.lru_cache(maxsize=None)
def window_expected(name, iters=25, top_max=5):
    """(top codes, scores, n_abnormal, n_normal, (resid_normal, resid_anomaly)) of the oracle's whole
    window with `iters` PageRank iterations (test_gpu_rca._oracle_rca with the count as an argument)."""
    na, nn, gs = window_graphs(name)
    res, resid = {}, []
    for g, anomaly in zip(gs, (False, True)):
        v = orc.preference(g, orc.trace_kinds(g), anomaly)
        s = orc.power_iteration(g, v, iters=iters)
        prev = orc.power_iteration(g, v, iters=iters - 1) if iters > 1 else np.ones(g.N) / float(g.N + g.T)
        resid.append(float(np.max(np.abs(s - prev))))
        res[anomaly] = orc.weights(g, s)
    top, score, _ = orc.spectrum(res[True][0], res[False][0], nn, na, top_max, res[False][1], res[True][1], "dstar2")
    return list(top), np.array(score, np.float64), na, nn, tuple(resid)
