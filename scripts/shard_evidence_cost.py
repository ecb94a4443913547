"""What the sharded evidence entries cost on one MI355X (DESIGN §3 "sharded evidence").

One process, a one-rank RCCL communicator (tests/test_gpu_shard.py::test_one_rank_rccl_matches_whole_graph's
set-up), the graph synth.big_graph(10_000, 1_250_000, seed=3): C4's 1/8 share.  Medians of 15 calls,
each bracketed by HIP events on the context stream:

  (a) mr_pagerank_sharded(iters=25) under this tree's library and under another build of it
      (--parent-lib: the commit before), processes alternating -- the one bar: within the +-3 %
      box-to-box spread of DESIGN §4;
  (b) mr_pagerank_sharded_converge(tol=1e-9, check_every=5, max_iters=200) against
      mr_pagerank_sharded with the count it stopped at;
  (c) one mr_graph_exemplars_sharded call for the 16 heaviest ops with m = 8;
  (d) the same answer from the downloaded vector (mr_graph_trace_rank_sharded, then numpy's selection
      over the ops' rows, the rows prepared beforehand).

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the
run.  The parent process prepares the graph and never opens the GPU.

    python3 scripts/shard_evidence_cost.py [--parent-lib PATH] [--out profiles/shard_evidence.json]
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

from converge_cost import Events  # noqa: E402  (scripts/ is sys.path[0] when this file runs)

CALLS, WARMUP = 15, 3
D, ALPHA, PHI = 0.85, 0.01, 0.5
TOL, CHECK, MAX_ITERS = 1e-9, 5, 200
EX_OPS, EX_M = 16, 8


def child(step, graph_file):
    import numpy as np
    import torch.distributed as dist

    from microrank_amd import _lib, shard
    from microrank_amd._lib import ptr
    from microrank_amd.graph import DeviceGraph

    with open(graph_file, "rb") as f:
        hg = pickle.load(f)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29531"))
    dist.init_process_group("gloo", rank=0, world_size=1)
    lib = _lib.load()
    ctx = _lib.default_context()
    shard.use_rccl(ctx)
    dg = DeviceGraph.upload(ctx, hg)
    ev = Events(lib.mr_ctx_stream(ctx.h))
    last = {}

    def plain(iters):
        def run():
            ctx.check(lib.mr_pagerank_sharded(ctx.h, dg.h, 1, D, ALPHA, iters, _lib.MR_FP64, 0), "mr_pagerank_sharded")
        return run

    runs = {"plain25": plain(25)}
    if step == "evidence":
        done, conv = C.c_int32(0), C.c_int32(0)
        resid = np.zeros(MAX_ITERS)

        def converge():
            ctx.check(lib.mr_pagerank_sharded_converge(ctx.h, dg.h, 1, D, ALPHA, MAX_ITERS, PHI, _lib.MR_FP64, 0, TOL, CHECK,
                                                       C.byref(done), ptr(resid, C.c_double), C.byref(conv)),
                      "mr_pagerank_sharded_converge")
            last.update(iters=int(done.value), converged_at=int(conv.value), last_residual=float(resid[done.value - 1]))

        converge()
        w, _ = dg.fetch()
        ops = np.argsort(-w, kind="stable")[:EX_OPS].astype(np.int32)
        order = np.argsort(hg.sr_ops, kind="stable")   # the asked ops' P_sr rows, prepared outside the timing
        trace_of = np.repeat(np.arange(hg.T, dtype=np.int64), np.diff(hg.sr_off))[order]
        start = np.searchsorted(hg.sr_ops[order], np.arange(hg.N + 1))
        rows = [trace_of[start[o]:start[o + 1]] for o in ops]
        tr, sc, cnt = np.empty((EX_OPS, EX_M), np.int64), np.empty((EX_OPS, EX_M)), np.empty(EX_OPS, np.int32)
        r, gid = np.empty(hg.T), np.empty(hg.T, np.int64)
        host = {}

        def exemplars():
            ctx.check(lib.mr_graph_exemplars_sharded(dg.h, ptr(ops, C.c_int32), EX_OPS, EX_M, ptr(tr, C.c_int64),
                                                     ptr(sc, C.c_double), ptr(cnt, C.c_int32)), "mr_graph_exemplars_sharded")

        def download():
            ctx.check(lib.mr_graph_trace_rank_sharded(dg.h, ptr(r, C.c_double), ptr(gid, C.c_int64)),
                      "mr_graph_trace_rank_sharded")
            for i, row in enumerate(rows):
                host[i] = gid[row[np.lexsort((row, -r[row]))[:EX_M]]]

        runs.update({"converge": converge, "plain_at_stop": plain(last["iters"])})
    times = {k: [] for k in runs}
    for k in range(WARMUP + CALLS):   # the forms alternate inside one process
        for name, fn in runs.items():
            ms, wall = ev.time_ms(fn)
            if k >= WARMUP:
                times[name].append((ms, wall))
    if step == "evidence":   # after the last ranking above: the exemplar call, then the download, alternating
        times.update(exemplars=[], download=[])
        for k in range(WARMUP + CALLS):
            for name, fn in (("exemplars", exemplars), ("download", download)):
                ms, wall = ev.time_ms(fn)
                if k >= WARMUP:
                    times[name].append((ms, wall))
        last["same_answer"] = all(host[i].tolist() == tr[i, :cnt[i]].tolist() for i in range(EX_OPS))
    res = {"step": step, "lib": os.path.basename(_lib.LIB_PATH), "N": hg.N, "T": hg.T, "nnz": int(hg.sr_ops.size)}
    for name, v in times.items():
        res[name] = {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
                     "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}
    res.update(last)
    print("RESULT " + json.dumps(res), flush=True)
    dg.close()
    ctx.close()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=10_000)
    ap.add_argument("--traces", type=int, default=1_250_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (a)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shard_evidence.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--dry", action="store_true", help="prepare the graph and stop (no GPU)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--graph", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.graph)
    from microrank_amd import synth

    hg = synth.big_graph(a.ops, a.traces, seed=3)
    print("graph:", (hg.N, hg.T, int(hg.sr_ops.size)), flush=True)
    if a.dry:
        return
    steps = [("evidence", None)]
    if a.parent_lib:
        steps += [("plain", None), ("plain", a.parent_lib)] * 2
    out = {"calls": CALLS, "warmup": WARMUP, "tol": TOL, "check_every": CHECK, "ex_ops": EX_OPS, "ex_m": EX_M, "steps": []}
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
    if a.parent_lib:
        for lib in sorted({s["lib"] for s in out["steps"][1:]}):
            out[f"a_plain25_ms_{lib}"] = [s["plain25"]["event_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
    evd = out["steps"][0]
    out["b_converge_over_fixed_count"] = evd["converge"]["event_ms_median"] / evd["plain_at_stop"]["event_ms_median"]
    out["d_download_over_exemplars_host"] = evd["download"]["host_ms_median"] / evd["exemplars"]["host_ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "steps"}), flush=True)


if __name__ == "__main__":
    main()
