"""Host side of the PageRank graph: dicts <-> incidence arrays <-> device handle.

``trace_pagerank`` receives the four dicts of ``get_pagerank_graph``
(preprocess_data.py:146-171).  Two ways in:

* the dicts are :class:`GraphDicts` views produced by this package's
  ``get_pagerank_graph`` -- they carry the device graph built by K1, nothing is converted;
* any other mapping -- it is turned into index arrays here, with the same lookups (and
  the same ``ValueError`` on an unknown key) as the reference's dense matrix fill
  (pagerank.py:26-52), then uploaded.
"""
from __future__ import annotations

import ctypes as C
import sys
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import GraphDesc, ptr


def _not_in_list(x) -> ValueError:
    return ValueError(f"{x!r} is not in list")


@dataclass
class HostGraph:
    nodes: list
    traces: list
    sr_off: np.ndarray      # int64 [T+1]
    sr_ops: np.ndarray      # int32
    rs_off: Optional[np.ndarray]
    rs_ops: Optional[np.ndarray]
    len_t: np.ndarray       # int32 [T]
    len_o: np.ndarray       # int32 [N]
    ss_off: np.ndarray      # int64 [N+1]
    ss_par: np.ndarray      # int32
    nchild: np.ndarray      # int32 [N]
    pr_trace: Optional[np.ndarray]   # int32, None = pr_trace is operation_trace
    pr_len: Optional[np.ndarray]

    @property
    def N(self):
        return len(self.nodes)

    @property
    def T(self):
        return len(self.traces)


def _csr(major: np.ndarray, minor: np.ndarray, n_major: int, n_minor: int):
    """Distinct (major, minor) pairs -> CSR with minors ascending."""
    if major.size == 0:
        return np.zeros(n_major + 1, np.int64), np.zeros(0, np.int32)
    key = np.unique(major.astype(np.int64) * max(n_minor, 1) + minor)
    maj = key // max(n_minor, 1)
    off = np.zeros(n_major + 1, np.int64)
    np.cumsum(np.bincount(maj, minlength=n_major), out=off[1:])
    return off, (key % max(n_minor, 1)).astype(np.int32)


def host_graph_from_dicts(operation_operation: Mapping, operation_trace: Mapping, trace_operation: Mapping,
                          pr_trace: Mapping) -> HostGraph:
    nodes = list(operation_operation.keys())
    traces = list(operation_trace.keys())
    ni = {k: i for i, k in enumerate(nodes)}
    ti = {k: i for i, k in enumerate(traces)}
    N, T = len(nodes), len(traces)

    def nget(x):
        try:
            return ni[x]
        except (KeyError, TypeError):
            raise _not_in_list(x) from None

    def tget(x):
        try:
            return ti[x]
        except (KeyError, TypeError):
            raise _not_in_list(x) from None

    # P_ss (pagerank.py:35-39): edge (child, parent), weight 1/len(children multiset of parent)
    nchild = np.zeros(N, np.int32)
    cs, ps = [], []
    for p, ch in operation_operation.items():
        pi = nget(p)
        nchild[pi] = len(ch)
        for c in ch:
            cs.append(nget(c))
            ps.append(pi)
    ss_off, ss_par = _csr(np.asarray(cs, np.int64), np.asarray(ps, np.int64), N, N)
    # P_sr (pagerank.py:42-45)
    len_t = np.fromiter((len(v) for v in operation_trace.values()), np.int32, count=T)
    flat = np.fromiter((nget(o) for v in operation_trace.values() for o in v), np.int64, count=int(len_t.sum()))
    sr_off, sr_ops = _csr(np.repeat(np.arange(T, dtype=np.int64), len_t), flat, T, N)
    # P_rs (pagerank.py:48-52)
    len_o = np.zeros(N, np.int32)
    rt, ro = [], []
    for o, trs in trace_operation.items():
        idx = [tget(t) for t in trs]   # trace looked up before the op, as at :52
        oi = nget(o)
        len_o[oi] = len(trs)
        rt.extend(idx)
        ro.extend([oi] * len(idx))
    rs_off, rs_ops = _csr(np.asarray(rt, np.int64), np.asarray(ro, np.int64), T, N)
    if rs_ops.size == sr_ops.size and np.array_equal(rs_off, sr_off) and np.array_equal(rs_ops, sr_ops):
        rs_off = rs_ops = None
    # pr_trace (pagerank.py:70-85)
    if pr_trace is operation_trace or (list(pr_trace.keys()) == traces and
                                       all(len(pr_trace[k]) == len_t[i] for i, k in enumerate(traces))):
        pr_t = pr_l = None
    else:
        pr_t = np.fromiter((tget(k) for k in pr_trace), np.int32, count=len(pr_trace))
        pr_l = np.fromiter((len(v) for v in pr_trace.values()), np.int32, count=len(pr_trace))
    return HostGraph(nodes, traces, sr_off, sr_ops, rs_off, rs_ops, len_t, len_o, ss_off, ss_par, nchild,
                     pr_t, pr_l)


def check_converge_args(tol, max_iters, check_every, phi=0.5) -> None:
    """The argument rules of mr_pagerank_converge, raised as ValueError before any library call."""
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)):
        raise ValueError(f"tol must be a number >= 0, not {tol!r}")
    if not float(tol) >= 0.0:   # (a NaN fails the comparison)
        raise ValueError(f"tol must be >= 0 and not NaN, not {tol!r}")
    for name, v in (("max_iters", max_iters), ("check_every", check_every)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, not {v!r}")
    if not float(phi) > 0.0:
        raise ValueError(f"phi must be > 0, not {phi!r}")


EX_MAX_OPS, EX_MAX_M = 64, 32   # mr_graph_exemplars: ops per call, traces per op


def check_exemplar_m(m) -> int:
    """mr_graph_exemplars' m, raised as ValueError before any library call."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= EX_MAX_M:
        raise ValueError(f"m must be an integer in 1..{EX_MAX_M}, not {m!r}")
    return int(m)


def check_exemplar_kinds(exemplar_kinds, exemplars) -> bool:
    """The exemplar_kinds keyword (one exemplar per trace kind) of the entries whose exemplars are
    optional: it needs exemplars=; raised as ValueError before any library call."""
    if not isinstance(exemplar_kinds, (bool, np.bool_)):
        raise ValueError(f"exemplar_kinds must be a bool, not {exemplar_kinds!r}")
    if exemplar_kinds and exemplars is None:
        raise ValueError("exemplar_kinds=True needs exemplars=m")
    return bool(exemplar_kinds)


def check_exemplar_ops(ops) -> list:
    """The ops of an exemplar request as a non-empty list (a lone name or index is not a list of them)."""
    if isinstance(ops, (str, bytes)) or not hasattr(ops, "__iter__"):
        raise ValueError(f"ops must be a sequence of node names or indices, not {ops!r}")
    ops = list(ops)
    if not ops:
        raise ValueError("ops is empty")
    return ops


def converge_batch(ctx, graphs, anomaly, *, tol: float, max_iters: int = 200, check_every: int = 5, d: float = 0.85,
                   alpha: float = 0.01, phi: float = 0.5, precision: str = "fp64", exact_sums: bool = False):
    """mr_pagerank_converge over several DeviceGraphs (anomaly: one flag per graph): the power
    iteration with each iteration's residual max|s_k - s_{k-1}| recorded on the device, stopped at
    the first check (every check_every iterations, and at max_iters) where every graph's last
    residual is <= tol.  Returns one dict per graph: ``iters`` (iterations every graph ran),
    ``residuals`` (ndarray[iters]) and ``converged_at`` (first k, 1-based, with residuals[k-1] <= tol,
    or None).  The weights are then those of a plain ranking with ``iters`` iterations, bit for bit."""
    check_converge_args(tol, max_iters, check_every, phi)
    graphs, anomaly = list(graphs), [int(bool(a)) for a in anomaly]
    if not graphs or len(graphs) != len(anomaly):
        raise ValueError("converge_batch: one anomaly flag per graph, at least one graph")
    lib = _lib.load()
    n = len(graphs)
    hs = (_lib.P * n)(*[g.h for g in graphs])
    an = (C.c_int * n)(*anomaly)
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    flags = _lib.MR_PR_EXACT_SUMS if exact_sums else 0
    done = C.c_int32(0)
    resid = np.zeros((n, int(max_iters)), np.float64)
    conv = np.empty(n, np.int32)
    ctx.check(lib.mr_pagerank_converge(ctx.h, hs, an, n, float(d), float(alpha), int(max_iters), float(phi), prec, flags,
                                       float(tol), int(check_every), C.byref(done), ptr(resid, C.c_double),
                                       ptr(conv, C.c_int32)), "mr_pagerank_converge")
    k = int(done.value)
    return [{"iters": k, "residuals": resid[i, :k].copy(), "converged_at": int(conv[i]) if conv[i] > 0 else None}
            for i in range(n)]


class DeviceGraph:
    """An mr_graph handle (HBM-resident incidence lists) plus the host-side names."""

    def __init__(self, ctx: "_lib.Context", handle, nodes, traces, N: int, T: int):
        self.ctx = ctx
        self.h = handle
        self.nodes = nodes
        self.traces = traces
        self.N = N
        self.T = T

    @classmethod
    def upload(cls, ctx, hg: HostGraph) -> "DeviceGraph":
        lib = _lib.load()
        d = GraphDesc()
        d.n_nodes, d.n_traces = hg.N, hg.T
        keep = [np.ascontiguousarray(a) for a in (hg.sr_off, hg.sr_ops, hg.len_t, hg.len_o, hg.ss_off,
                                                  hg.ss_par, hg.nchild)]
        d.nnz_sr = int(hg.sr_ops.size)
        d.sr_off, d.sr_ops = ptr(keep[0], C.c_int64), ptr(keep[1], C.c_int32)
        d.len_t, d.len_o = ptr(keep[2], C.c_int32), ptr(keep[3], C.c_int32)
        d.n_edges = int(hg.ss_par.size)
        d.ss_off, d.ss_par, d.nchild = ptr(keep[4], C.c_int64), ptr(keep[5], C.c_int32), ptr(keep[6], C.c_int32)
        if hg.rs_off is not None:
            keep += [np.ascontiguousarray(hg.rs_off), np.ascontiguousarray(hg.rs_ops)]
            d.nnz_rs = int(hg.rs_ops.size)
            d.rs_off, d.rs_ops = ptr(keep[-2], C.c_int64), ptr(keep[-1], C.c_int32)
        if hg.pr_trace is not None:
            keep += [np.ascontiguousarray(hg.pr_trace), np.ascontiguousarray(hg.pr_len)]
            d.n_pr = int(hg.pr_trace.size)
            d.pr_trace, d.pr_len = ptr(keep[-2], C.c_int32), ptr(keep[-1], C.c_int32)
        else:
            d.n_pr = hg.T
        h = _lib.P()
        ctx.check(lib.mr_graph_upload(ctx.h, C.byref(d), C.byref(h)), "mr_graph_upload")
        return cls(ctx, h, hg.nodes, hg.traces, hg.N, hg.T)

    def pagerank(self, anomaly: bool, d: float = 0.85, alpha: float = 0.01, iters: int = 25,
                 precision: str = "fp64", exact_sums: bool = False, compress_kinds: bool = False,
                 phi: float = 0.5):
        """compress_kinds: iterate over one representative trace per kind (pagerank.py:54-66 --
        traces of a kind have identical r), the multiplicities carried; same weights.  phi: the
        anomaly preference's weight (pagerank.py:82-84)."""
        lib = _lib.load()
        prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
        flags = (_lib.MR_PR_EXACT_SUMS if exact_sums else 0) | (_lib.MR_PR_KIND_COMPRESS if compress_kinds else 0)
        if iters < 0:
            raise ValueError("iters must be >= 0")
        self.ctx.check(lib.mr_pagerank_ex(self.ctx.h, self.h, int(bool(anomaly)), float(d), float(alpha), int(iters),
                                          float(phi), prec, flags), "mr_pagerank_ex")

    def converge(self, anomaly: bool, *, tol: float, max_iters: int = 200, check_every: int = 5, d: float = 0.85,
                 alpha: float = 0.01, phi: float = 0.5, precision: str = "fp64", exact_sums: bool = False):
        """Rank to a tolerance (converge_batch for this graph alone): {"iters", "residuals", "converged_at"}."""
        return converge_batch(self.ctx, [self], [anomaly], tol=tol, max_iters=max_iters, check_every=check_every, d=d,
                              alpha=alpha, phi=phi, precision=precision, exact_sums=exact_sums)[0]

    def fetch(self, kinds: bool = False):
        lib = _lib.load()
        w = np.empty(self.N, np.float64)
        cov = np.empty(self.N, np.int32)
        kind = np.empty(self.T, np.float64) if kinds else None
        pref = np.empty(self.T, np.float32) if kinds else None
        self.ctx.check(lib.mr_graph_fetch(self.h, ptr(w, C.c_double), ptr(cov, C.c_int32),
                                          ptr(kind, C.c_double), ptr(pref, C.c_float)), "mr_graph_fetch")
        return (w, cov, kind, pref) if kinds else (w, cov)

    def trace_rank(self) -> np.ndarray:
        """The trace half of the last ranking: ndarray[T] (float64) of what the reference holds in
        request_ranking_vector after its iterations (pagerank.py:119-127), in this graph's trace order."""
        r = np.empty(self.T, np.float64)
        self.ctx.check(_lib.load().mr_graph_trace_rank(self.h, ptr(r, C.c_double)), "mr_graph_trace_rank")
        return r

    def _node_indices(self, ops) -> list:
        index = None
        out = []
        for op in ops:
            if isinstance(op, (int, np.integer)) and not isinstance(op, bool):
                if not 0 <= op < self.N:
                    raise ValueError(f"op index {op!r} outside [0, {self.N})")
                out.append(int(op))
                continue
            if index is None:
                index = {k: i for i, k in enumerate(self.nodes)}
            try:
                out.append(index[op])
            except (KeyError, TypeError):
                raise ValueError(f"unknown op {op!r}") from None
        return out

    def exemplars_raw(self, idx, m: int, distinct_kinds: bool = False):
        """mr_graph_exemplars for node indices (any number: calls of EX_MAX_OPS): (traces [n, m] int32,
        -1 padded; scores [n, m]; counts [n]).  distinct_kinds (mr_graph_exemplars_ex with
        MR_EX_DISTINCT_KINDS): one trace per trace kind, and a 4th array, the kinds' class sizes
        [n, m] int32, 0 padded."""
        lib = _lib.load()
        n = len(idx)
        tr = np.empty((n, m), np.int32)
        sc = np.empty((n, m), np.float64)
        cnt = np.empty(n, np.int32)
        mult = np.empty((n, m), np.int32) if distinct_kinds else None
        for b in range(0, n, EX_MAX_OPS):
            ops = np.asarray(idx[b:b + EX_MAX_OPS], np.int32)
            k = int(ops.size)
            t, s, c = np.empty((k, m), np.int32), np.empty((k, m), np.float64), np.empty(k, np.int32)
            if distinct_kinds:
                mu = np.empty((k, m), np.int32)
                self.ctx.check(lib.mr_graph_exemplars_ex(self.h, ptr(ops, C.c_int32), k, m, _lib.MR_EX_DISTINCT_KINDS,
                                                         ptr(t, C.c_int32), ptr(s, C.c_double), ptr(c, C.c_int32),
                                                         ptr(mu, C.c_int32)), "mr_graph_exemplars_ex")
                mult[b:b + k] = mu
            else:
                self.ctx.check(lib.mr_graph_exemplars(self.h, ptr(ops, C.c_int32), k, m, ptr(t, C.c_int32),
                                                      ptr(s, C.c_double), ptr(c, C.c_int32)), "mr_graph_exemplars")
            tr[b:b + k], sc[b:b + k], cnt[b:b + k] = t, s, c
        return (tr, sc, cnt, mult) if distinct_kinds else (tr, sc, cnt)

    def exemplars(self, ops, m: int = 5, distinct_kinds: bool = False) -> dict:
        """For each op (node names or indices) the m traces that matter most to the last ranking among
        the traces the op occurs in (its operation_trace row): {op: [(trace, score), ...]} in request
        order, score descending, ties by trace order; trace is the trace's name (its index on a graph
        without names), score its entry of trace_rank().  distinct_kinds: one trace per trace kind
        (traces with the same operations and span count: the ranking's own classes), each kind by its
        best trace, as (trace, score, count) with count the number of traces of that kind in the graph."""
        m = check_exemplar_m(m)
        ops = check_exemplar_ops(ops)
        idx = self._node_indices(ops)
        names = self.traces
        out = {}
        if distinct_kinds:
            tr, sc, cnt, mult = self.exemplars_raw(idx, m, True)
            for i, op in enumerate(ops):
                out[op] = [(names[int(t)] if names is not None else int(t), np.float64(s), int(c))
                           for t, s, c in zip(tr[i, :cnt[i]], sc[i, :cnt[i]], mult[i, :cnt[i]])]
            return out
        tr, sc, cnt = self.exemplars_raw(idx, m)
        for i, op in enumerate(ops):
            out[op] = [(names[int(t)] if names is not None else int(t), np.float64(s))
                       for t, s in zip(tr[i, :cnt[i]], sc[i, :cnt[i]])]
        return out

    def info(self):
        n, t, nnz, e = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        _lib.load().mr_graph_info(self.h, C.byref(n), C.byref(t), C.byref(nnz), C.byref(e))
        return dict(N=n.value, T=t.value, nnz=nnz.value, E=e.value)

    def close(self):
        # a destroyed context has freed its handles already (mr_ctx_destroy)
        if getattr(self, "h", None) and getattr(getattr(self, "ctx", None), "h", None):
            _lib.load().mr_graph_free(self.h)
        self.h = None

    def __del__(self):  # pragma: no cover
        if sys.is_finalizing():   # the owning context may already be destroyed
            return
        try:
            self.close()
        except Exception:
            pass
