"""What one exemplar per trace kind costs on one MI355X (DESIGN §3 "K2 exemplars").

The C2-shaped graph of scripts/exemplar_cost.py (tests/gpu_util.c2_graph: 1000 ops, 200k traces), every
trace selected, ranked with 25 iterations; 16 ops from the most covered down, m = 8.  Medians of 15
calls, each bracketed by HIP events on the context stream (and by the host's clock: the entries end in
a read-back):

  (a) mr_graph_exemplars_ex with MR_EX_DISTINCT_KINDS on the cached trace vector and representatives,
      beside mr_graph_exemplars (the plain call) in the same process; the graph's first distinct call
      (the kinds' representatives are computed there, once per graph) is timed apart;
  (b) the plain call and mr_pagerank_batch(iters=25) under this tree's library and under another build
      of it (--parent-lib: the commit before), processes alternating.

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the run.
The parent process prepares the graph and never opens the GPU.

    python3 scripts/exemplar_kinds_cost.py [--parent-lib PATH] [--out profiles/exemplar_kinds.json]
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from converge_cost import Events  # noqa: E402  (scripts/ is sys.path[0])
from exemplar_cost import ALPHA, CALLS, D, M, N_OPS, WARMUP, host_graph, summary  # noqa: E402


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
    res = {"step": step, "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
           "N": hg.N, "T": hg.T, "nnz": int(hg.sr_ops.size)}
    cov = np.bincount(hg.sr_ops, minlength=hg.N)
    ops = np.argsort(-cov, kind="stable")[:: max(1, hg.N // N_OPS)][:N_OPS].astype(np.int32)
    tr, sc, cnt = np.empty((N_OPS, M), np.int32), np.empty((N_OPS, M), np.float64), np.empty(N_OPS, np.int32)
    mu = np.empty((N_OPS, M), np.int32)

    def rank():
        ctx.check(lib.mr_pagerank_batch(ctx.h, hs, an, 1, D, ALPHA, 25, _lib.MR_FP64, 0), "mr_pagerank_batch")

    def plain():
        ctx.check(lib.mr_graph_exemplars(dg.h, ptr(ops, C.c_int32), N_OPS, M, ptr(tr, C.c_int32), ptr(sc, C.c_double),
                                         ptr(cnt, C.c_int32)), "mr_graph_exemplars")

    def distinct():
        ctx.check(lib.mr_graph_exemplars_ex(dg.h, ptr(ops, C.c_int32), N_OPS, M, _lib.MR_EX_DISTINCT_KINDS,
                                            ptr(tr, C.c_int32), ptr(sc, C.c_double), ptr(cnt, C.c_int32),
                                            ptr(mu, C.c_int32)), "mr_graph_exemplars_ex")

    times = {"rank": [], "plain_cached": []}
    if step == "kinds":
        times["distinct_cached"] = []
        rank()
        plain()                                  # (the trace vector is cached from here)
        res["distinct_first_call"] = dict(zip(("event_ms", "host_ms"), ev.time_ms(distinct)))
    for i in range(WARMUP + CALLS):
        a = ev.time_ms(rank)
        plain()
        b = ev.time_ms(plain)
        c = None
        if step == "kinds":
            distinct()
            c = ev.time_ms(distinct)
        if i >= WARMUP:
            times["rank"].append(a)
            times["plain_cached"].append(b)
            if c is not None:
                times["distinct_cached"].append(c)
    for k, v in times.items():
        res[k] = summary(v)
    if step == "kinds":
        kind = dg.fetch(kinds=True)[2]
        res.update(kinds=int(round(float((1.0 / kind).sum()))), entries=int(cnt.sum()),
                   class_size_max=int(mu.max()), ops=[int(o) for o in ops], coverage=[int(cov[o]) for o in ops])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (b)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exemplar_kinds.json"))
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--dry", action="store_true", help="prepare the graph (and write it to --graph) and stop: no GPU")
    ap.add_argument("--child", default=None)
    ap.add_argument("--graph", default=None, help="a pickled host graph (written by --dry --graph PATH) instead of building it")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.graph)
    if a.graph and not a.dry:
        with open(a.graph, "rb") as f:
            hg = pickle.load(f)
    else:
        hg = host_graph(a.ops, a.traces)
    print("graph:", (hg.N, hg.T, int(hg.sr_ops.size)), flush=True)
    if a.dry:
        if a.graph:
            with open(a.graph, "wb") as f:
                pickle.dump(hg, f)
        return
    steps = [("kinds", None)]
    if a.parent_lib:
        steps += [("base", None), ("base", a.parent_lib)] * 3
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
            res = json.loads(line[len("RESULT "):])
            res["which"] = "parent" if libpath else "this"
            out["steps"].append(res)
    k = out["steps"][0]
    out["a_distinct_over_plain"] = k["distinct_cached"]["event_ms_median"] / k["plain_cached"]["event_ms_median"]
    if a.parent_lib:
        for which in ("this", "parent"):
            base = [s for s in out["steps"][1:] if s["which"] == which]
            out[f"b_plain_ms_{which}"] = [s["plain_cached"]["event_ms_median"] for s in base]
            out[f"b_rank_ms_{which}"] = [s["rank"]["event_ms_median"] for s in base]
        for key in ("plain", "rank"):
            t, p_ = (statistics.median(out[f"b_{key}_ms_{w}"]) for w in ("this", "parent"))
            out[f"b_{key}_this_over_parent"] = t / p_
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "steps"}), flush=True)


if __name__ == "__main__":
    main()
