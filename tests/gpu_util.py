"""Helpers shared by the tests: oracle graphs -> product host graphs, golden -> dicts, and the
generator of general graphs (general_graph) with its dict form (graph_dicts)."""
import numpy as np

import oracle as orc
from microrank_amd.graph import HostGraph, _csr


def host_graph_from_oracle(g: "orc.Graph") -> HostGraph:
    N, T = g.N, g.T
    sr_off, sr_ops = _csr(g.sr_t, g.sr_o, T, N)
    rs_off, rs_ops = _csr(g.rs_t, g.rs_o, T, N)
    same = np.array_equal(sr_off, rs_off) and np.array_equal(sr_ops, rs_ops)
    ss_off, ss_par = _csr(g.ss_c, g.ss_p, N, N)
    ident = np.array_equal(g.pr_idx, np.arange(T)) and np.array_equal(g.pr_len, g.len_t)
    return HostGraph(list(g.nodes), list(g.traces), sr_off, sr_ops, None if same else rs_off,
                     None if same else rs_ops, g.len_t.astype(np.int32), g.len_o.astype(np.int32), ss_off,
                     ss_par, g.nchild.astype(np.int32), None if ident else g.pr_idx.astype(np.int32),
                     None if ident else g.pr_len.astype(np.int32))


def golden_graph_dicts(exp, tnames):
    """Compact golden graph (make_golden.dump_graph) -> the four reference dicts."""
    nodes = exp["nodes"]

    def unflat(d, kname, vname):
        out = {}
        pos = 0
        for k, ln in zip(d["keys"], d["len"]):
            out[kname(k)] = [vname(v) for v in d["vals"][pos:pos + ln]]
            pos += ln
        return out

    oo = unflat(exp["operation_operation"], lambda i: nodes[i], lambda i: nodes[i])
    ot = unflat(exp["operation_trace"], lambda i: tnames[i], lambda i: nodes[i])
    to = unflat(exp["trace_operation"], lambda i: nodes[i], lambda i: tnames[i])
    return oo, ot, to, dict(ot)


def _pairs(major, minor, n_minor):
    """Distinct (major, minor) pairs sorted by (major, minor), as two int64 arrays."""
    key = np.unique(np.asarray(major, np.int64) * n_minor + np.asarray(minor, np.int64))
    return key // n_minor, key % n_minor


def general_graph(N, T, seed, *, zipf=1.1, mean_len=12, empty_frac=0.02, multiset=0.2, rs_drop=0.1, rs_add=0.05,
                  pr_frac=0.7, edges_per_node=3, long_trace=0) -> "orc.Graph":
    """A graph of the general form trace_pagerank accepts, not the form get_pagerank_graph builds.

    * op popularity Zipf(``zipf``) over a random order of the ops, Poisson(``mean_len``) draws per trace
      (at least one), the distinct ops of the draws kept;
    * ``empty_frac`` of the traces have no op (len_t = 0);
    * ``multiset`` of the traces / ops / parents that have entries count 1..3 more than their distinct
      entries in len_t / len_o / nchild (an entity without entries keeps 0: the graph has a dict form);
    * P_rs is P_sr with ``rs_drop`` of the pairs removed and ``rs_add`` (of the pair count) random pairs
      added; both 0: the same arrays;
    * pr_idx is the first ``pr_frac`` of a random permutation of the traces, pr_len random in 1..29;
      ``pr_frac=None``: pr_trace is operation_trace (then use empty_frac=0: 1/len of an empty list);
    * about ``edges_per_node`` * N random call edges, self loops allowed;
    * ``long_trace=k``: trace T // 2 has k distinct ops (T counts it).
    """
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, N + 1, dtype=np.float64) ** zipf
    p = (p / p.sum())[rng.permutation(N)]
    draws = np.maximum(rng.poisson(mean_len, T), 1)
    n_empty = int(round(empty_frac * T))
    draws[rng.permutation(T)[:n_empty]] = 0
    if long_trace:
        draws[T // 2] = 0
    t_of = np.repeat(np.arange(T, dtype=np.int64), draws)
    o_of = rng.choice(N, size=int(draws.sum()), p=p)
    if long_trace:
        t_of = np.concatenate([t_of, np.full(long_trace, T // 2, np.int64)])
        o_of = np.concatenate([o_of, rng.choice(N, size=long_trace, replace=False)])
    sr_t, sr_o = _pairs(t_of, o_of, N)
    nnz = sr_t.size
    if rs_drop or rs_add:
        keep = rng.random(nnz) >= rs_drop
        if rs_drop and keep.all():   # (a handful of pairs: still not the transpose)
            keep[rng.integers(nnz)] = False
        n_add = int(round(rs_add * nnz))
        rs_t, rs_o = _pairs(np.concatenate([sr_t[keep], rng.integers(0, T, n_add)]),
                            np.concatenate([sr_o[keep], rng.integers(0, N, n_add)]), N)
    else:
        rs_t, rs_o = sr_t, sr_o
    n_e = edges_per_node * N
    ss_c, ss_p = _pairs(rng.integers(0, N, n_e), rng.integers(0, N, n_e), N)

    def lengths(distinct):
        extra = np.where(rng.random(distinct.size) < multiset, rng.integers(1, 4, distinct.size), 0)
        return (distinct + np.where(distinct > 0, extra, 0)).astype(np.int64)

    len_t = lengths(np.bincount(sr_t, minlength=T))
    len_o = lengths(np.bincount(rs_o, minlength=N))
    nchild = lengths(np.bincount(ss_p, minlength=N))
    if pr_frac is None:
        pr_idx, pr_len = np.arange(T, dtype=np.int64), len_t.copy()
    else:
        pr_idx = rng.permutation(T)[:max(1, int(round(pr_frac * T)))].astype(np.int64)
        pr_len = rng.integers(1, 30, pr_idx.size).astype(np.int64)
    return orc.Graph([f"o{i}" for i in range(N)], [f"t{i}" for i in range(T)], sr_t, sr_o, rs_t, rs_o, len_t, len_o,
                     ss_c, ss_p, nchild, pr_idx, pr_len)


def graph_dicts(g: "orc.Graph"):
    """The four dicts whose orc.graph_from_dicts is ``g`` again, array for array: a list holds its
    distinct entries in index order, then its first entry again for each count above the distinct
    ones; ops without P_rs entries are no key of trace_operation; pr_trace's lists hold len copies
    of the first node (only their lengths are read, pagerank.py:70-85)."""
    nodes, traces = list(g.nodes), list(g.traces)

    def lists(major, minor, n_major, length, names):
        cnt = np.bincount(major, minlength=n_major)
        assert ((length >= cnt) & ((cnt > 0) | (length == 0))).all(), "no dict form"
        out, pos = [], 0
        for i in range(n_major):
            ent = [names[j] for j in minor[pos:pos + cnt[i]]]
            pos += cnt[i]
            out.append(ent + ent[:1] * int(length[i] - cnt[i]))
        return out

    by_p = np.lexsort((g.ss_c, g.ss_p))
    oo = dict(zip(nodes, lists(g.ss_p[by_p], g.ss_c[by_p], g.N, g.nchild, nodes)))
    ot = dict(zip(traces, lists(g.sr_t, g.sr_o, g.T, g.len_t, nodes)))
    by_o = np.lexsort((g.rs_t, g.rs_o))
    to_all = lists(g.rs_o[by_o], g.rs_t[by_o], g.N, g.len_o, traces)
    to = {n: v for n, v in zip(nodes, to_all) if v}
    pt = {traces[t]: [nodes[0]] * int(ln) for t, ln in zip(g.pr_idx, g.pr_len)}
    return oo, ot, to, pt


def general_golden_dicts(fix):
    """tests/golden/dict_general.json's recorded input (make_golden.dict_general) -> the four dicts."""
    nodes, traces = fix["nodes"], fix["traces"]

    def unflat(d, knames, vnames):
        out, pos = {}, 0
        for k, ln in zip(d["keys"], d["len"]):
            out[knames[k]] = [vnames[v] for v in d["vals"][pos:pos + ln]]
            pos += ln
        return out

    return (unflat(fix["operation_operation"], nodes, nodes), unflat(fix["operation_trace"], traces, nodes),
            unflat(fix["trace_operation"], nodes, traces), unflat(fix["pr_trace"], traces, nodes))


def c2_graph(n_ops=1000, n_traces=200_000, seed=7, anomaly_split=True):
    """A C2-shaped window graph built by the oracle from synthetic spans."""
    from microrank_amd import synth

    topo = synth.make_topology(n_ops, seed)
    st = synth.gen_spans(topo, n_traces, seed + 1, branch=1.9, p_max=0.8, names=False)
    sel = np.ones(n_traces, dtype=bool)
    sg = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel)
    return st, sg
