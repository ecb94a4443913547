"""Reference values for the exemplar tests, derived from oracle functions alone (oracle/ returns only
the operation vector s): the trace vector the reference holds in request_ranking_vector after K
iterations (pagerank.py:119-127), and numpy's selection of an op's top traces."""
import numpy as np

import oracle as orc

D = 0.85


def trace_rank_ref(g, v, K, d=D):
    """r_K, max-normalised (K = 0: the un-normalised 1/(N+T) of pagerank.py:119).
    r_K = d * P_rs s_{K-1} + fp32((1-d) v) over its maximum (:125, :127), s_{K-1} the oracle's
    max-normalised iterate (s_0 = 1/(N+T), :118)."""
    N, T = g.N, g.T
    if K == 0:
        return np.full(T, 1.0 / float(N + T))
    s_prev = orc.power_iteration(g, v, d=d, iters=K - 1) if K >= 2 else np.full(N, 1.0 / float(N + T))
    w_rs = (1.0 / np.maximum(g.len_o, 1)).astype(np.float32).astype(np.float64)[g.rs_o]
    c = ((1.0 - d) * v.astype(np.float32)).astype(np.float64)
    r = d * np.bincount(g.rs_t, weights=w_rs * s_prev[g.rs_o], minlength=T) + c
    return r / np.max(r)


def two_vector_pagerank(g, v, K, d=D, alpha=0.01):
    """pagerank.py:116-130 restated plainly over the incidence lists, both vectors carried:
    (s, r) as the reference holds them after K iterations."""
    N, T = g.N, g.T
    w_sr = (1.0 / np.maximum(g.len_t, 1)).astype(np.float32).astype(np.float64)
    w_rs = (1.0 / np.maximum(g.len_o, 1)).astype(np.float32).astype(np.float64)
    w_ss = (1.0 / np.maximum(g.nchild, 1)).astype(np.float32).astype(np.float64)
    s = np.ones(N) / float(N + T)
    r = np.ones(T) / float(N + T)
    c = ((1.0 - d) * v.astype(np.float32)).astype(np.float64)
    for _ in range(K):
        s_new = np.zeros(N)
        np.add.at(s_new, g.sr_o, w_sr[g.sr_t] * r[g.sr_t])
        ss = np.zeros(N)
        np.add.at(ss, g.ss_c, w_ss[g.ss_p] * s[g.ss_p])
        r_new = np.zeros(T)
        np.add.at(r_new, g.rs_t, w_rs[g.rs_o] * s[g.rs_o])
        s_new = d * (s_new + alpha * ss)
        r_new = d * r_new + c
        s = s_new / np.max(s_new)
        r = r_new / np.max(r_new)
    return s, r


def top_traces(row, r, m):
    """The first min(m, len(row)) traces of an op's P_sr row: score descending, index ascending on ties."""
    row = np.asarray(row, np.int64)
    order = np.lexsort((row, -r[row]))
    return row[order[:m]]


def rows_by_op(sr_t, sr_o, N):
    """P_sr rows: for each op the ascending trace indices of the (trace, op) pairs."""
    order = np.lexsort((sr_t, sr_o))
    cnt = np.bincount(sr_o, minlength=N)
    off = np.zeros(N + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    t = np.asarray(sr_t, np.int64)[order]
    return [t[off[o]:off[o + 1]] for o in range(N)]
