"""Drop-in for the reference module ``pagerank`` (pagerank.py).

``trace_pagerank(operation_operation, operation_trace, trace_operation, pr_trace, anomaly)``
returns ``(weight, trace_num_list)`` exactly like pagerank.py:15-112: two dicts in node
order, weights as ``np.float64``, coverage counts as ``int``.  The work runs on the GPU
(K2 in microrank_amd/csrc/mr_pagerank.hip and mr_pr_*.hip: a file map is in DESIGN.md §3); nothing is computed on the host
except the dict <-> index conversion for mappings that did not come from this package's
``get_pagerank_graph``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .graph import DeviceGraph, check_converge_args, host_graph_from_dicts

D, ALPHA, ITERATIONS = 0.85, 0.01, 25   # pagerank.py:116-117
PHI = 0.5                               # pagerank.py:82-84 (the anomaly preference's two 0.5s)
MAX_ITERS = 200                         # tol= without max_iters=


class _DefaultIters(int):
    """The iters default: the reference's 25 as a value, recognised by identity so that an
    explicit iters= beside tol= can be refused."""


_ITERS_DEFAULT = _DefaultIters(ITERATIONS)


def _device_graph(operation_operation, operation_trace, trace_operation, pr_trace, ctx):
    from .preprocess_data import GraphDicts

    if isinstance(operation_operation, GraphDicts) and operation_operation.owner is not None:
        own = operation_operation.owner
        if (operation_trace is own.operation_trace and trace_operation is own.trace_operation and
                pr_trace is own.pr_trace):
            return own.device_graph(), False
    hg = host_graph_from_dicts(operation_operation, operation_trace, trace_operation, pr_trace)
    if hg.N == 0 or hg.T == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    return DeviceGraph.upload(ctx, hg), True


def trace_pagerank(operation_operation, operation_trace, trace_operation, pr_trace, anomaly, *,
                   d: float = D, alpha: float = ALPHA, iters: int = _ITERS_DEFAULT, phi: float = PHI,
                   precision: str = "fp64", ctx=None, compress_kinds: bool = False,
                   tol: float = None, max_iters: int = None, check_every: int = 5, info: dict = None,
                   trace_result: dict = None):
    """pagerank.trace_pagerank on MI355X (pagerank.py:15-112).  The reference hard-codes d, alpha
    (pageRank's defaults, :116), the 25 iterations (:117) and phi (:82-84); they are keywords here
    with the reference's values as defaults.  compress_kinds: rank one representative per trace
    kind with its multiplicity (same weights within fp64 rounding).

    tol: iterate until max|s_k - s_{k-1}| <= tol instead of a fixed count (the reference's README
    asks for more iterations on large systems), looked at every check_every iterations and at
    max_iters (default 200); a dict passed as info receives ``iters``, ``residuals`` and
    ``converged_at`` (DeviceGraph.converge).  Not together with iters= or compress_kinds.

    trace_result: a dict passed here receives {trace name: np.float64(r)} in trace order -- the trace
    half of the ranking, which the reference computes and drops (request_ranking_vector,
    pagerank.py:119-127; DeviceGraph.trace_rank).  Not with compress_kinds."""
    if trace_result is not None:
        if not isinstance(trace_result, dict):
            raise ValueError("trace_result must be a dict (or None)")
        if compress_kinds:
            raise ValueError("trace_result= with compress_kinds=True is not supported: the trace vector of a "
                             "kind-compressed ranking (MR_PR_KIND_COMPRESS) lives on the kinds' representatives")
    if tol is None:
        if max_iters is not None:
            raise ValueError("max_iters needs tol (a fixed count is iters=)")
        iters = int(iters)
    else:
        if iters is not _ITERS_DEFAULT:
            raise ValueError("iters= and tol= exclude each other: with tol the count is max_iters")
        if compress_kinds:
            raise ValueError("tol= with compress_kinds=True is not supported: mr_pagerank_converge has no "
                             "kind-compressed form (MR_PR_KIND_COMPRESS)")
        max_iters = MAX_ITERS if max_iters is None else max_iters
        check_converge_args(tol, max_iters, check_every, phi)
        if info is not None and not isinstance(info, dict):
            raise ValueError("info must be a dict (or None)")
    ctx = ctx or _lib.default_context()
    g, owned = _device_graph(operation_operation, operation_trace, trace_operation, pr_trace, ctx)
    try:
        if tol is None:
            g.pagerank(bool(anomaly), d, alpha, iters, precision, compress_kinds=compress_kinds, phi=phi)
        else:
            rep = g.converge(bool(anomaly), tol=tol, max_iters=max_iters, check_every=check_every, d=d, alpha=alpha,
                             phi=phi, precision=precision)
            if info is not None:
                info.update(rep)
        w, cov = g.fetch()
        if trace_result is not None:
            r = g.trace_rank()
            for i, name in enumerate(g.traces if g.traces is not None else operation_trace.keys()):
                trace_result[name] = np.float64(r[i])
    finally:
        if owned:
            g.close()
    nodes = g.nodes
    weight = {}
    trace_num_list = {}
    for i, op in enumerate(nodes):
        trace_num_list[op] = int(cov[i])
    for i, op in enumerate(nodes):
        weight[op] = np.float64(w[i])
    return weight, trace_num_list
