"""What the convergence report costs on one MI355X (DESIGN §3 "convergence").

A C2-shaped pair: the spans of tests/gpu_util.c2_graph (1000 ops, 200k traces), their traces split
in two halves, the first ranked as the normal graph and the second as the anomaly graph in one
batch.  Medians of 15 calls, each bracketed by HIP events on the context stream:

  (a) mr_pagerank_batch(iters=25) against mr_pagerank_converge(tol=0, max_iters=25): the
      per-iteration cost of k_resid plus the k_fx_b launch form (no pf launches);
  (b) mr_pagerank_converge(tol=1e-9, check_every=5, max_iters=200): iterations run and time;
  (c) mr_pagerank_batch(iters=25) under this tree's library and under another build of it
      (--parent-lib: the commit before), processes alternating.

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the
run.  The parent process prepares the graphs and never opens the GPU.

    python3 scripts/converge_cost.py [--parent-lib PATH] [--out profiles/pagerank_converge.json]
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

CALLS, WARMUP = 15, 3
D, ALPHA, PHI = 0.85, 0.01, 0.5


def host_graphs(n_ops, n_traces):
    import numpy as np

    import oracle as orc
    from gpu_util import c2_graph, host_graph_from_oracle

    st, _ = c2_graph(n_ops, n_traces)
    out = []
    for half in (0, 1):
        sel = np.zeros(n_traces, dtype=bool)
        sel[half::2] = True
        out.append(host_graph_from_oracle(orc.span_graph(st.trace, st.podop, st.span, st.parent, sel).as_graph()))
    return out


class Events:
    """Two HIP events around a call on the context stream."""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time_ms(self, fn):
        assert self.hip.hipEventRecord(self.ev[0], self.stream) == 0
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        assert self.hip.hipEventRecord(self.ev[1], self.stream) == 0
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float(0.0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return float(ms.value), wall


def child(step, graphs_file):
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    with open(graphs_file, "rb") as f:
        hgs = pickle.load(f)
    lib = _lib.load()
    ctx = _lib.default_context()
    dgs = [DeviceGraph.upload(ctx, hg) for hg in hgs]
    n = len(dgs)
    hs = (_lib.P * n)(*[dg.h for dg in dgs])
    an = (C.c_int * n)(0, 1)
    ev = Events(lib.mr_ctx_stream(ctx.h))
    last = {}

    def plain():
        ctx.check(lib.mr_pagerank_batch(ctx.h, hs, an, n, D, ALPHA, 25, _lib.MR_FP64, 0), "mr_pagerank_batch")

    def converge(tol, max_iters, every):
        done = C.c_int32(0)
        resid = (C.c_double * (n * max_iters))()
        conv = (C.c_int32 * n)()

        def run():
            ctx.check(lib.mr_pagerank_converge(ctx.h, hs, an, n, D, ALPHA, max_iters, PHI, _lib.MR_FP64, 0, tol, every,
                                               C.byref(done), resid, conv), "mr_pagerank_converge")
            last.update(iters=done.value, converged_at=list(conv),
                        last_residuals=[resid[i * max_iters + done.value - 1] for i in range(n)])
        return run

    runs = {"plain": plain}
    if step == "converge":
        runs["tol0"] = converge(0.0, 25, 5)
        runs["tol1e-9"] = converge(1e-9, 200, 5)
    times = {k: [] for k in runs}
    for r in range(WARMUP + CALLS):   # the forms alternate inside one process
        for k, fn in runs.items():
            ms, wall = ev.time_ms(fn)
            if r >= WARMUP:
                times[k].append((ms, wall))
    res = {"step": step, "lib": os.path.basename(_lib.LIB_PATH), "N": [hg.N for hg in hgs], "T": [hg.T for hg in hgs]}
    for k, v in times.items():
        res[k] = {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
                  "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}
    if step == "converge":
        res["tol1e-9"].update(last)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (c)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pagerank_converge.json"))
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--dry", action="store_true", help="prepare the graphs and stop (no GPU)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--graphs", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.graphs)
    hgs = host_graphs(a.ops, a.traces)
    print("graphs:", [(hg.N, hg.T, int(hg.sr_ops.size)) for hg in hgs], flush=True)
    if a.dry:
        return
    steps = [("converge", None)]
    if a.parent_lib:
        steps += [("plain", None), ("plain", a.parent_lib)] * 2
    out = {"calls": CALLS, "warmup": WARMUP, "steps": []}
    with tempfile.TemporaryDirectory() as tmp:
        gf = os.path.join(tmp, "graphs.pkl")
        with open(gf, "wb") as f:
            pickle.dump(hgs, f)
        for step, libpath in steps:
            env = dict(os.environ)
            env.pop("MR_LIB_PATH", None)
            if libpath:
                env["MR_LIB_PATH"] = os.path.abspath(libpath)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step,
                   "--graphs", gf]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            if p.returncode != 0:   # nothing more on the GPU after a step that failed
                print(f"step {step} ({libpath or 'this tree'}) ended with status {p.returncode}", flush=True)
                sys.exit(p.returncode)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            out["steps"].append(json.loads(line[len("RESULT "):]))
    conv = out["steps"][0]
    out["a_per_iteration_cost_us"] = (conv["tol0"]["event_ms_median"] - conv["plain"]["event_ms_median"]) * 1e3 / 25
    if a.parent_lib:
        for lib in sorted({s["lib"] for s in out["steps"][1:]}):
            out[f"c_plain_ms_{lib}"] = [s["plain"]["event_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "steps"}), flush=True)


if __name__ == "__main__":
    main()
