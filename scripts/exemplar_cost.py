"""What the exemplar entries cost on one MI355X (DESIGN §3 "K2 exemplars").

A C2-shaped graph: the spans of tests/gpu_util.c2_graph (1000 ops, 200k traces), every trace selected,
ranked with 25 iterations.  Medians of 15 calls, each bracketed by HIP events on the context stream
(and by the host's clock: the entries end in a read-back, so the host time is what a caller waits):

  (a) mr_graph_trace_rank right after a ranking (k_trace_rank + the 8 T byte download) and again (the
      cached vector: the download alone); mr_graph_exemplars with 16 ops and m = 8 on the cached vector
      and right after a ranking (k_trace_rank first);
  (b) the host form of the same answer: mr_graph_export + the fetched r + numpy's per-op top-m;
  (c) the byte floor: one read of the P_sr ids as stored (2 B each for N <= 65536) plus 8 T bytes of
      the vector, over mr_copy_peak's measured rate;
  (d) mr_pagerank_batch(iters=25) on the same graph under this tree's library and under another build
      of it (--parent-lib: the commit before), processes alternating.

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the
run.  The parent process prepares the graph and never opens the GPU.

    python3 scripts/exemplar_cost.py [--parent-lib PATH] [--out profiles/exemplars.json]
"""
import argparse
import ctypes as C
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from converge_cost import Events  # noqa: E402  (scripts/ is sys.path[0])

CALLS, WARMUP = 15, 3
D, ALPHA = 0.85, 0.01
N_OPS, M = 16, 8


def host_graph(n_ops, n_traces):
    from gpu_util import c2_graph, host_graph_from_oracle

    _, sg = c2_graph(n_ops, n_traces)
    return host_graph_from_oracle(sg.as_graph())


def summary(v):
    return {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
            "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}


def child(step, graph_file):
    import numpy as np

    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.graph import DeviceGraph

    with open(graph_file, "rb") as f:
        hg = pickle.load(f)
    lib = _lib.load()
    ctx = _lib.default_context()
    dg = DeviceGraph.upload(ctx, hg)
    hs = (_lib.P * 1)(dg.h)
    an = (C.c_int * 1)(1)
    ev = Events(lib.mr_ctx_stream(ctx.h))
    res = {"step": step, "lib": os.path.basename(_lib.LIB_PATH), "N": hg.N, "T": hg.T, "nnz": int(hg.sr_ops.size)}

    def rank():
        ctx.check(lib.mr_pagerank_batch(ctx.h, hs, an, 1, D, ALPHA, 25, _lib.MR_FP64, 0), "mr_pagerank_batch")

    if step == "plain":
        t = []
        for r in range(WARMUP + CALLS):
            x = ev.time_ms(rank)
            if r >= WARMUP:
                t.append(x)
        res["plain"] = summary(t)
        print("RESULT " + json.dumps(res), flush=True)
        return

    cov = np.bincount(hg.sr_ops, minlength=hg.N)
    ops = np.argsort(-cov, kind="stable")[:: max(1, hg.N // N_OPS)][:N_OPS].astype(np.int32)   # from the most covered down
    r = np.empty(hg.T, np.float64)
    tr, sc, cnt = np.empty((N_OPS, M), np.int32), np.empty((N_OPS, M), np.float64), np.empty(N_OPS, np.int32)

    def trace_rank():
        ctx.check(lib.mr_graph_trace_rank(dg.h, ptr(r, C.c_double)), "mr_graph_trace_rank")

    def exemplars():
        ctx.check(lib.mr_graph_exemplars(dg.h, ptr(ops, C.c_int32), N_OPS, M, ptr(tr, C.c_int32), ptr(sc, C.c_double),
                                         ptr(cnt, C.c_int32)), "mr_graph_exemplars")

    off, ids = np.empty(hg.T + 1, np.int64), np.empty(hg.sr_ops.size, np.int32)
    host_out = {}

    def host_form():
        ctx.check(lib.mr_graph_export(dg.h, ptr(off, C.c_int64), ptr(ids, C.c_int32), None, None, None, None, None),
                  "mr_graph_export")
        trace_rank()
        t_of = np.repeat(np.arange(hg.T, dtype=np.int64), np.diff(off))
        for o in ops:
            row = t_of[ids == o]
            order = np.lexsort((row, -r[row]))[:M]
            host_out[int(o)] = (row[order], r[row][order])

    times = {k: [] for k in ("trace_rank_fresh", "trace_rank_cached", "exemplars_cached", "exemplars_fresh", "host_form")}
    for i in range(WARMUP + CALLS):
        rank()
        a = ev.time_ms(trace_rank)
        b = ev.time_ms(trace_rank)
        c = ev.time_ms(exemplars)
        rank()
        d = ev.time_ms(exemplars)
        e = ev.time_ms(host_form)
        if i >= WARMUP:
            for k, x in zip(times, (a, b, c, d, e)):
                times[k].append(x)
    for j, o in enumerate(ops):   # the two forms answer alike
        n = int(cnt[j])
        assert n == min(M, int(cov[o])) and tr[j, :n].tolist() == host_out[int(o)][0].tolist()
        assert sc[j, :n].tobytes() == host_out[int(o)][1].tobytes()
    for k, v in times.items():
        res[k] = summary(v)
    gbs = C.c_double(0.0)
    ctx.check(lib.mr_copy_peak(ctx.h, 256 << 20, 5, C.byref(gbs)), "mr_copy_peak")
    id_bytes = 2 if hg.N <= 65536 else 4
    floor_bytes = id_bytes * int(hg.sr_ops.size) + 8 * hg.T
    res.update(copy_peak_gbs=gbs.value, id_bytes=id_bytes, floor_bytes=floor_bytes,
               floor_us=floor_bytes / (gbs.value * 1e3), ops=[int(o) for o in ops], coverage=[int(cov[o]) for o in ops])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (d)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exemplars.json"))
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--dry", action="store_true", help="prepare the graph and stop (no GPU)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--graph", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.graph)
    hg = host_graph(a.ops, a.traces)
    print("graph:", (hg.N, hg.T, int(hg.sr_ops.size)), flush=True)
    if a.dry:
        return
    steps = [("exemplars", None)]
    if a.parent_lib:
        steps += [("plain", None), ("plain", a.parent_lib)] * 3
    out = {"calls": CALLS, "warmup": WARMUP, "n_ops": N_OPS, "m": M, "steps": []}
    with tempfile.TemporaryDirectory() as tmp:
        gf = os.path.join(tmp, "graph.pkl")
        with open(gf, "wb") as f:
            pickle.dump(hg, f)
        for step, libpath in steps:
            env = dict(os.environ)
            env.pop("MR_LIB_PATH", None)
            if libpath:
                env["MR_LIB_PATH"] = os.path.abspath(libpath)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step,
                   "--graph", gf]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            if p.returncode != 0:   # nothing more on the GPU after a step that failed
                print(f"step {step} ({libpath or 'this tree'}) ended with status {p.returncode}", flush=True)
                sys.exit(p.returncode)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            out["steps"].append(json.loads(line[len("RESULT "):]))
    ex = out["steps"][0]
    kern_us = (ex["trace_rank_fresh"]["event_ms_median"] - ex["trace_rank_cached"]["event_ms_median"]) * 1e3
    out["a_trace_rank_kernel_us"] = kern_us
    out["b_host_over_device"] = ex["host_form"]["host_ms_median"] / ex["exemplars_fresh"]["host_ms_median"]
    out["c_floor_fraction_exemplars_cached"] = ex["floor_us"] / (ex["exemplars_cached"]["event_ms_median"] * 1e3)
    if a.parent_lib:
        for lib in sorted({s["lib"] for s in out["steps"][1:]}):
            out[f"d_plain_ms_{lib}"] = [s["plain"]["event_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "steps"}), flush=True)


if __name__ == "__main__":
    main()
