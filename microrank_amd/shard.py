"""Trace-sharded PageRank over several processes.

One process per GPU holds a shard of the traces (every span of a trace on one rank) over the
global node index space.  ``mr_pagerank_sharded`` (csrc/mr_pagerank.hip, csrc/mr_pr_shard.hip; the kernels' exchange modes: csrc/mr_pr_fxb_dev.h)
exchanges, once per graph, the per-op span counts / children counts / coverage, the call edges and the trace-kind
classes, and per iteration ONE all-reduce: the exact fixed-point P_sr r limbs (uint64 SUM) with
every rank's max r' in a one-hot slot, so every rank ends with the weights the whole graph would
give.  :func:`build_graph` builds a rank's graph from its span shard (K1 over the ranks: global
node order, cross-rank parent joins).

Collectives run over RCCL (:func:`use_rccl`, xGMI between GPUs) or, for ranks that share a GPU
or have no RCCL, over a host-staged callback on a ``torch.distributed`` process group
(:func:`use_host`; gloo in the tests).  torch is the control plane only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr

HOST_COLL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int)
_NP = {0: np.float64, 1: np.int32, 2: np.int64, 3: np.int64}   # uint64 reduced as int64: same bits
                                                                 # for sums mod 2^64 and for the
                                                                 # max of non-negative values


class _HostCollectives:
    """mr_host_coll_fn over a torch.distributed group; keeps the ctypes callback alive."""

    def __init__(self, group=None):
        import torch.distributed as dist

        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.fn = HOST_COLL(self._call)

    def _call(self, user, coll, buf, n, dtype, op):
        import torch

        try:
            dt = _NP[dtype]
            if coll == 0:
                a = np.ctypeslib.as_array((C.c_byte * (n * np.dtype(dt).itemsize)).from_address(buf)).view(dt)
                t = torch.from_numpy(a.copy())
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX if op else self.dist.ReduceOp.SUM, group=self.group)
                a[:] = t.numpy()
            else:
                a = np.ctypeslib.as_array(
                    (C.c_byte * (n * self.world * np.dtype(dt).itemsize)).from_address(buf)).view(dt)
                mine = torch.from_numpy(a[self.rank * n:(self.rank + 1) * n].copy())
                parts = [torch.empty_like(mine) for _ in range(self.world)]
                self.dist.all_gather(parts, mine, group=self.group)
                a[:] = torch.cat(parts).numpy()
            return 0
        except Exception:   # never raise through C
            return 1


def use_host(ctx: "_lib.Context", group=None):
    """Host-staged collectives over a torch.distributed group (any backend, e.g. gloo)."""
    hc = _HostCollectives(group)
    ctx.check(_lib.load().mr_comm_set_host(ctx.h, C.cast(hc.fn, C.c_void_p), None, hc.world, hc.rank),
              "mr_comm_set_host")
    ctx._host_coll = hc
    return hc


def use_rccl(ctx: "_lib.Context", group=None):
    """RCCL communicator for this context: rank 0's unique id travels over the torch group."""
    import torch
    import torch.distributed as dist

    lib = _lib.load()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    uid = np.zeros(128, np.uint8)
    if rank == 0:
        ctx.check(lib.mr_comm_unique_id(ptr(uid, C.c_uint8)), "mr_comm_unique_id")
    t = torch.from_numpy(uid.copy())
    dist.broadcast(t, src=0, group=group)
    uid[:] = t.numpy()
    ctx.check(lib.mr_comm_init(ctx.h, world, rank, ptr(uid, C.c_uint8)), "mr_comm_init")


def use_peer(ctx: "_lib.Context", enable: bool = True):
    """The per-iteration all-reduce through IPC-mapped peer memory (mr_comm_peer_enable): one
    push of this rank's limbs into every rank's receive region, one local sum -- instead of the
    RCCL / host-staged all-reduce.  Needs a collective backend first (use_rccl / use_host) for the
    one-time exchange of the IPC handles."""
    ctx.check(_lib.load().mr_comm_peer_enable(ctx.h, int(bool(enable))), "mr_comm_peer_enable")


def peer_active(ctx: "_lib.Context") -> bool:
    """True while the peer path carries this context's all-reduces (its regions mapped on every
    rank); False before the first sharded call, or after the ranks fell back to RCCL / the host
    collective (a failed mapping, a peer timeout)."""
    a = C.c_int32()
    ctx.check(_lib.load().mr_comm_peer_active(ctx.h, C.byref(a)), "mr_comm_peer_active")
    return bool(a.value)


def sharded_pagerank(dg, anomaly: bool, d: float = 0.85, alpha: float = 0.01, iters: int = 25,
                     precision: str = "fp64"):
    """PageRank of the whole graph from this rank's shard ``dg`` (a DeviceGraph whose len_o /
    nchild are this rank's partial counts and whose call edges are its local ones).  Returns
    (weights, coverage) of the whole graph, identical on every rank."""
    lib = _lib.load()
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    dg.ctx.check(lib.mr_pagerank_sharded(dg.ctx.h, dg.h, int(bool(anomaly)), d, alpha, iters, prec, 0),
                 "mr_pagerank_sharded")
    return dg.fetch()


def build_graph(dev_spans, trace_mask) -> "DeviceGraph":
    """K1 on this rank's span shard (mr_graph_build_sharded): ``dev_spans`` holds every span of
    this rank's traces with global codes and global row indices (SpanTable.shard);
    ``trace_mask`` selects the trace_list over the global trace codes.  The graph has the whole
    graph's node order (T10) and its cross-rank parent joins (T11); its len_o / nchild / edges are
    this rank's parts, which :func:`sharded_pagerank` combines."""
    from .graph import DeviceGraph

    lib = _lib.load()
    ctx = dev_spans.ctx
    mask = np.ascontiguousarray(trace_mask, dtype=np.uint8)
    h = _lib.P()
    ctx.check(lib.mr_graph_build_sharded(ctx.h, dev_spans.h, ptr(mask, C.c_uint8), C.byref(h)),
              "mr_graph_build_sharded")
    n, t, nnz, e = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    lib.mr_graph_info(h, C.byref(n), C.byref(t), C.byref(nnz), C.byref(e))
    node_podop = np.empty(n.value, np.int32)
    trace_code = np.empty(t.value, np.int32)
    ctx.check(lib.mr_graph_nodes(h, ptr(node_podop, C.c_int32), ptr(trace_code, C.c_int32)), "mr_graph_nodes")
    return DeviceGraph(ctx, h, node_podop, trace_code, n.value, t.value)


def sharded_converge(dg, anomaly: bool, *, tol: float, max_iters: int = 200, check_every: int = 5, d: float = 0.85,
                     alpha: float = 0.01, phi: float = 0.5, precision: str = "fp64"):
    """:func:`sharded_pagerank` to a tolerance (mr_pagerank_sharded_converge; collective: every rank
    calls it with the same arguments, differing ones raise ValueError on every rank).  Every
    iteration's residual max|s_k - s_{k-1}| of the WHOLE graph is recorded on the device; at every
    check (check_every iterations, and at max_iters) the ranks agree on the words and stop where the
    last residual is <= tol.  Returns (weights, coverage, {"iters", "residuals", "converged_at"}), the
    dict as DeviceGraph.converge's and identical on every rank; the weights are those of
    ``sharded_pagerank(iters=iters)``, bit for bit."""
    from .graph import check_converge_args

    check_converge_args(tol, max_iters, check_every, phi)
    lib = _lib.load()
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    done = C.c_int32(0)
    conv = C.c_int32(-1)
    resid = np.zeros(int(max_iters), np.float64)
    dg.ctx.check(lib.mr_pagerank_sharded_converge(dg.ctx.h, dg.h, int(bool(anomaly)), float(d), float(alpha),
                                                  int(max_iters), float(phi), prec, 0, float(tol), int(check_every),
                                                  C.byref(done), ptr(resid, C.c_double), C.byref(conv)),
                 "mr_pagerank_sharded_converge")
    k = int(done.value)
    w, cov = dg.fetch()
    return w, cov, {"iters": k, "residuals": resid[:k].copy(), "converged_at": int(conv.value) if conv.value > 0 else None}


def sharded_trace_rank(dg):
    """The trace half of the last sharded ranking for THIS rank's traces (mr_graph_trace_rank_sharded;
    not collective): (gid int64[T], r float64[T]).  r is normalised by the whole graph's maximum, so
    the ranks' vectors concatenate to the whole graph's request_ranking_vector; gid is each trace's
    global id -- its trace code on a graph of :func:`build_graph`, its index in the concatenation of
    the ranks' traces on an uploaded shard."""
    gid = np.empty(dg.T, np.int64)
    r = np.empty(dg.T, np.float64)
    dg.ctx.check(_lib.load().mr_graph_trace_rank_sharded(dg.h, ptr(r, C.c_double), ptr(gid, C.c_int64)),
                 "mr_graph_trace_rank_sharded")
    return gid, r


def sharded_exemplars(dg, ops, m: int = 5) -> dict:
    """For each op (node names or indices) the m traces of the WHOLE graph that matter most to the last
    sharded ranking among the traces the op occurs in (mr_graph_exemplars_sharded; collective: every
    rank calls it with the same ops and m): {op: [(global id, score), ...]}, score descending, global
    id ascending on equal scores, identical on every rank.  Global ids as :func:`sharded_trace_rank`'s."""
    from .graph import EX_MAX_OPS, check_exemplar_m, check_exemplar_ops

    m = check_exemplar_m(m)
    ops = check_exemplar_ops(ops)
    idx = dg._node_indices(ops)
    lib = _lib.load()
    out = {}
    for b in range(0, len(idx), EX_MAX_OPS):
        part = np.asarray(idx[b:b + EX_MAX_OPS], np.int32)
        k = int(part.size)
        tr, sc, cnt = np.empty((k, m), np.int64), np.empty((k, m), np.float64), np.empty(k, np.int32)
        dg.ctx.check(lib.mr_graph_exemplars_sharded(dg.h, ptr(part, C.c_int32), k, m, ptr(tr, C.c_int64),
                                                    ptr(sc, C.c_double), ptr(cnt, C.c_int32)),
                     "mr_graph_exemplars_sharded")
        for i in range(k):
            out[ops[b + i]] = [(int(t), np.float64(s)) for t, s in zip(tr[i, :cnt[i]], sc[i, :cnt[i]])]
    return out
