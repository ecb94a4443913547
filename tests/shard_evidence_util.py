"""What the sharded evidence tests share: spawned ranks on one GPU over gloo (a worker runs a named
scenario on its shard and returns plain arrays), the window graph's cuts, and the CPU oracle's
residual history.  Every worker initialises gloo with a 90 s timeout, catches its exception and puts it
in the queue; the parent reads with a timeout and retries nothing."""
import ctypes as C
import datetime
import functools
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle as orc
from test_dist_gloo import _shard, _window_graph

TOL, CHECK, MAX_ITERS = 3e-9, 5, 200   # the stop the converge tests ask for


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@functools.lru_cache(maxsize=None)
def window_graph():
    return _window_graph()


@functools.lru_cache(maxsize=None)
def preference(anomaly):
    g = window_graph()
    return orc.preference(g, orc.trace_kinds(g), anomaly)


@functools.lru_cache(maxsize=None)
def oracle_history(anomaly, n=60):
    """max|s_k - s_{k-1}|, k = 1..n, on the WHOLE graph (s_0 the un-normalised 1/(N+T))."""
    g, v = window_graph(), preference(anomaly)
    prev = np.full(g.N, 1.0 / float(g.N + g.T))
    out = np.empty(n)
    for k in range(1, n + 1):
        s = orc.power_iteration(g, v, iters=k)
        out[k - 1] = np.max(np.abs(s - prev))
        prev = s
    out.setflags(write=False)
    return out


def expected_stop(anomaly):
    """The first check (every CHECK iterations) where the oracle's residual is <= TOL, with a factor
    >= 1.5 between TOL and the residuals on both sides of the decision (tests/test_gpu_window_iters.py's rule)."""
    h = oracle_history(anomaly)
    k = next(k for k in range(CHECK, len(h) + 1, CHECK) if h[k - 1] <= TOL)
    assert h[k - 1] * 1.5 <= TOL and h[k - CHECK - 1] >= 1.5 * TOL, (k, h[k - 1], h[k - CHECK - 1])
    return k


def bounds_of(cut, T, world):
    if cut == "empty_last":
        return [0] + [T] * world    # rank 0 all traces, the rest none
    if cut == "uneven":
        assert world == 2
        return [0, 40, T]
    return [r * T // world for r in range(world)] + [T]


def exemplars_raw(dg, ops, m):
    """mr_graph_exemplars_sharded as it answers: (ids [n, m] int64, scores [n, m], counts [n]) or the status."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    ops = np.asarray(ops, np.int32)
    n = int(ops.size)
    tr, sc, cnt = np.full((n, max(m, 1)), -7, np.int64), np.full((n, max(m, 1)), -7.0), np.full(n, -7, np.int32)
    rc = _lib.load().mr_graph_exemplars_sharded(dg.h, ptr(ops, C.c_int32), n, m, ptr(tr, C.c_int64), ptr(sc, C.c_double),
                                                ptr(cnt, C.c_int32))
    return (tr, sc, cnt) if rc == 0 else rc


def converge_raw(dg, anomaly, flags=0, max_iters=10, tol=0.0, check_every=CHECK):
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    done = C.c_int32(0)
    resid = np.zeros(max_iters)
    return _lib.load().mr_pagerank_sharded_converge(dg.ctx.h, dg.h, int(anomaly), 0.85, 0.01, max_iters, 0.5, 0, flags, tol,
                                                    check_every, C.byref(done), ptr(resid, C.c_double), None)


# ------------------------------------------------------------------ scenarios (run inside a rank)
def sc_converge(dg, rank, world, opt):
    """Per preference: the 60-iteration history with the weights of the fixed count, then the stop."""
    from microrank_amd import shard

    out = {}
    for an in opt.get("anomaly", (False, True)):
        o = out[an] = {}
        if opt.get("history", True):
            w, cov, info = shard.sharded_converge(dg, an, tol=0.0, max_iters=60)
            o["hist"], o["hist_iters"], o["hist_conv"] = info["residuals"], info["iters"], info["converged_at"]
            o["hist_w_same"] = w.tobytes() == shard.sharded_pagerank(dg, an, iters=60)[0].tobytes()
        w, cov, info = shard.sharded_converge(dg, an, tol=TOL, check_every=CHECK, max_iters=MAX_ITERS)
        o["stop"], o["stop_hist"], o["stop_conv"], o["w"], o["cov"] = info["iters"], info["residuals"], info["converged_at"], w, cov
        o["stop_w_same"] = w.tobytes() == shard.sharded_pagerank(dg, an, iters=info["iters"])[0].tobytes()
        if opt.get("fp32"):
            o["hist32"] = shard.sharded_converge(dg, an, tol=0.0, max_iters=30, precision="fp32")[2]["residuals"]
    if opt.get("errors"):
        from microrank_amd import _lib

        e = out["errors"] = {}
        e["kind_compress"] = converge_raw(dg, True, flags=_lib.MR_PR_KIND_COMPRESS)
        try:   # rank 1 asks for another check_every: every rank must hear of it
            shard.sharded_converge(dg, True, tol=TOL, check_every=7 if rank == 1 else CHECK, max_iters=MAX_ITERS)
            e["disagree"] = "no error"
        except ValueError as x:
            e["disagree"] = "ValueError: " + str(x)
        e["after"] = shard.sharded_converge(dg, True, tol=TOL, check_every=CHECK, max_iters=MAX_ITERS)[2]["iters"]
    return out


def sc_exemplars(dg, rank, world, opt):
    """Per (preference, iterations): this rank's (gid, r) and the raw answers for all ops and each m."""
    from microrank_amd import _lib, shard
    from microrank_amd._lib import ptr

    out = {}
    ops = list(range(dg.N))
    if opt.get("errors"):
        e = out["errors"] = {}
        r = np.empty(dg.T)
        e["before_rank"] = _lib.load().mr_graph_trace_rank_sharded(dg.h, ptr(r, C.c_double), None)
        e["before_ex"] = exemplars_raw(dg, ops[:3], 4)
    for an, iters in opt.get("cases", [(a, k) for a in (False, True) for k in (25, 1)]):
        o = out[(an, iters)] = {}
        shard.sharded_pagerank(dg, an, iters=iters)
        o["gid"], o["r"] = shard.sharded_trace_rank(dg)
        for m in opt.get("ms", (1, 8, 32)):
            o[m] = exemplars_raw(dg, ops, m)
    if opt.get("blocks"):   # the cut into selection blocks must not show (read per call)
        os.environ["MR_EX_BLOCKS"] = "1"
        out["blocks1"] = exemplars_raw(dg, ops, 8)
        os.environ.pop("MR_EX_BLOCKS")
        out["blocks_default"] = exemplars_raw(dg, ops, 8)
    if opt.get("python"):   # the dict form against the raw answer it wraps (the last ranking above)
        d = shard.sharded_exemplars(dg, ops, m=8)
        tr, sc, cnt = exemplars_raw(dg, ops, 8)
        out["python_same"] = list(d) == ops and all(
            d[i] == [(int(t), s) for t, s in zip(tr[i, :cnt[i]], sc[i, :cnt[i]])] for i in ops)
    if opt.get("converge"):   # the record follows the iterations the converge call ran
        an = True
        w, cov, info = shard.sharded_converge(dg, an, tol=TOL, check_every=CHECK, max_iters=MAX_ITERS)
        a = shard.sharded_trace_rank(dg)[1]
        xa = exemplars_raw(dg, ops, 8)
        shard.sharded_pagerank(dg, an, iters=info["iters"])
        b = shard.sharded_trace_rank(dg)[1]
        xb = exemplars_raw(dg, ops, 8)
        out["converge"] = (info["iters"], a.tobytes() == b.tobytes(), all(x.tobytes() == y.tobytes() for x, y in zip(xa, xb)))
    if opt.get("errors"):
        e = out["errors"]
        e["m33"] = exemplars_raw(dg, ops[:3], 33)
        e["ops65"] = exemplars_raw(dg, [0] * 65, 4)
        e["disagree"] = exemplars_raw(dg, ops[:5], 3 if rank == 1 else 4)   # every rank must hear of it
        e["after"] = exemplars_raw(dg, ops[:5], 4)
        r = np.empty(dg.T)
        e["old_rank"] = _lib.load().mr_graph_trace_rank(dg.h, ptr(r, C.c_double))
        tr, sc, cnt = np.empty((1, 4), np.int32), np.empty((1, 4)), np.empty(1, np.int32)
        one = np.zeros(1, np.int32)
        e["old_ex"] = _lib.load().mr_graph_exemplars(dg.h, ptr(one, C.c_int32), 1, 4, ptr(tr, C.c_int32), ptr(sc, C.c_double),
                                                    ptr(cnt, C.c_int32))
    return out


def sc_span(dg, rank, world, opt):
    """A span-built shard (shard.build_graph): global ids are trace codes; mr_pagerank_converge still
    rejects it, mr_pagerank_sharded_converge ranks it."""
    from microrank_amd import shard
    from microrank_amd.graph import converge_batch

    out = {"trace_code": np.asarray(dg.traces), "nodes": np.asarray(dg.nodes)}
    try:
        converge_batch(dg.ctx, [dg], [True], tol=TOL)
        out["old_converge"] = "no error"
    except ValueError as x:
        out["old_converge"] = "ValueError: " + str(x)
    w, cov, info = shard.sharded_converge(dg, True, tol=TOL, check_every=CHECK, max_iters=MAX_ITERS)
    out["stop"] = info["iters"]
    out["stop_w_same"] = w.tobytes() == shard.sharded_pagerank(dg, True, iters=info["iters"])[0].tobytes()
    shard.sharded_pagerank(dg, True)
    out["gid"], out["r"] = shard.sharded_trace_rank(dg)
    out["ex"] = exemplars_raw(dg, list(range(min(dg.N, 64))), 8)
    return out


SCENARIOS = {"converge": sc_converge, "exemplars": sc_exemplars, "span": sc_span}


def _worker(rank, world, port, q, scenario, opt):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if opt.get("tile"):
        os.environ["MR_NO_FUSED"] = "1"   # read once, at this process's first graph prepare
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    try:
        from gpu_util import host_graph_from_oracle
        from microrank_amd import _lib, shard
        from microrank_amd.graph import DeviceGraph

        ctx = _lib.Context(0)
        if opt.get("backend") == "rccl":
            shard.use_rccl(ctx)
        else:
            shard.use_host(ctx)
        if opt.get("peer"):
            shard.use_peer(ctx)
        dev = None
        if scenario == "span":
            from microrank_amd.preprocess_data import DeviceSpans
            from test_gpu_shard import _span_mask, _span_table

            st = _span_table()
            dev = DeviceSpans(ctx, st.shard(rank, world))
            dg = shard.build_graph(dev, _span_mask(st))
        else:
            g = window_graph()
            dg = DeviceGraph.upload(ctx, host_graph_from_oracle(_shard(g, rank, world, bounds_of(opt.get("cut"), g.T, world))))
        out = SCENARIOS[scenario](dg, rank, world, opt)
        out["T"] = dg.T
        dg.close()
        if dev is not None:
            dev.close()
        ctx.close()
        q.put((rank, out, None))
    except Exception as e:   # surface the failure in the parent
        q.put((rank, None, repr(e)))
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def span_run():
    """The span-built pair, one spawned run for both test files."""
    return run(2, "span")


@functools.lru_cache(maxsize=None)
def whole_graph(anomaly, iters):
    """The whole window graph ranked on one GPU: (weights, coverage, trace_rank); computed once, left unchanged."""
    from gpu_util import host_graph_from_oracle
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    ctx = _lib.Context(0)
    dg = DeviceGraph.upload(ctx, host_graph_from_oracle(window_graph()))
    dg.pagerank(anomaly, iters=iters)
    w, cov = dg.fetch()
    r = dg.trace_rank()
    dg.close()
    ctx.close()
    return w, cov, r


def run(world, scenario, **opt):
    """The ranks' results in rank order (at most 4 processes on the GPU)."""
    assert world <= 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, scenario, opt)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out, err in res:
        assert err is None, f"rank {rank} failed: {err}"
    return [out for rank, out, err in sorted(res, key=lambda r: r[0])]
