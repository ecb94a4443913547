"""What the window entries' iteration count, report and tolerance cost on one MI355X (DESIGN §3
"K2 convergence", window batches).

Workload: a C2-shaped call of 8 windows (bench.c2_windows: 1000 ops / 200k traces each, one SLO
period) and one C3 window (bench.make_window(4242, 500, 20000)).  Medians of 15 calls, each bracketed
by HIP events on the context stream (the calls return drained, so the host's wall time is beside it):

  (a) the plain entries, mr_windows_batch (the 8 windows) and mr_rca_window (the C3 window), under
      this tree's library and under another build of it (--parent-lib: the commit before), processes
      alternating.  The plain entries are wrappers of the _ex entries now; a difference beyond the
      box-to-box spread would mean the wrapper changed the launches.
  (b) mr_windows_batch_ex / mr_rca_window_ex with a report at iters=25 against the plain entries in
      the same process: one k_resid launch per group, its words in the error words' copy.
  (c) the tol form (tol=1e-9, check_every=5, iters=200) against the fixed count at the iterations it
      ran, with a report: the price of ranking the groups synchronously.

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the
run.  The parent process generates the tables and never opens the GPU.

    python3 scripts/window_iters_cost.py [--parent-lib PATH] [--out profiles/window_iters.json]
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
for p in (REPO, os.path.join(REPO, "scripts")):
    sys.path.insert(0, p)

from converge_cost import Events   # noqa: E402

CALLS, WARMUP = 15, 3
TOL, EVERY, MAX_ITERS = 1e-9, 5, 200


def child(step, tables_file):
    import numpy as np

    import bench
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.preprocess_data import DeviceSpans

    with open(tables_file, "rb") as f:
        c2_normal, c2_tabs, c3_normal, c3_tab = pickle.load(f)
    lib = _lib.load()
    ctx = _lib.default_context()
    ev = Events(lib.mr_ctx_stream(ctx.h))
    five = 5 * 60 * 10**9

    def windows(normal, tabs):
        a3, ok = bench.slo_from_gpu(ctx, normal)
        return [(DeviceSpans(ctx, t), int(t.tstart.min()), int(t.tstart.min()) + five, a3, ok) for t in tabs]

    c2, c3 = windows(c2_normal, c2_tabs), windows(c3_normal, [c3_tab])[0]
    n = len(c2)
    spans = (_lib.P * n)(*[w[0].h for w in c2])
    t0, t1 = np.array([w[1] for w in c2], np.int64), np.array([w[2] for w in c2], np.int64)
    a3p, okp = (C.c_void_p * n)(*[w[3].ctypes.data for w in c2]), (C.c_void_p * n)(*[w[4].ctypes.data for w in c2])
    codes, scores = np.zeros(n * 11, np.int32), np.zeros(n * 11)
    n_out, na, nn, status = (np.zeros(n, np.int32) for _ in range(4))
    edges = np.zeros(n, np.int64)
    done, resid = np.zeros(n, np.int32), np.zeros(2 * n)
    last = {}

    def batch_args():
        return (ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3p, okp, 0, 5, _lib.MR_FP64, ptr(codes, C.c_int32),
                ptr(scores, C.c_double), ptr(n_out, C.c_int32), ptr(edges, C.c_int64), ptr(na, C.c_int32),
                ptr(nn, C.c_int32), ptr(status, C.c_int32))

    o1, e1, a1, b1 = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
    d1, r1 = np.zeros(1, np.int32), np.zeros(2)

    def one_args():
        dev, u0, u1, s3, sok = c3
        return (ctx.h, dev.h, u0, u1, ptr(s3, C.c_double), ptr(sok, C.c_uint8), 0, 5, _lib.MR_FP64, ptr(codes, C.c_int32),
                ptr(scores, C.c_double), C.byref(o1), C.byref(e1), C.byref(a1), C.byref(b1))

    # (the argument lists are converted once, outside the timed calls: a single window's call is
    # latency-bound and a ctypes conversion costs microseconds)
    b_args, o_args = batch_args(), one_args()
    b_rep, o_rep = (ptr(done, C.c_int32), ptr(resid, C.c_double)), (ptr(d1, C.c_int32), ptr(r1, C.c_double))
    seen = {}   # key -> the report of its last call, read after the timed loop

    def batch_ex(key, iters, tol):
        seen[key] = lambda: {"iters": done.tolist(), "resid_max": float(resid.max())}
        return lambda: ctx.check(lib.mr_windows_batch_ex(*b_args, iters, tol, EVERY, *b_rep), "mr_windows_batch_ex")

    def one_ex(key, iters, tol):
        seen[key] = lambda: {"iters": d1.tolist(), "resid_max": float(r1.max())}
        return lambda: ctx.check(lib.mr_rca_window_ex(*o_args, iters, tol, EVERY, *o_rep), "mr_rca_window_ex")

    runs = {"batch_plain": lambda: ctx.check(lib.mr_windows_batch(*b_args), "mr_windows_batch"),
            "one_plain": lambda: ctx.check(lib.mr_rca_window(*o_args), "mr_rca_window")}
    if step == "ex":
        runs["batch_report25"] = batch_ex("batch_report25", 25, 0.0)
        runs["one_report25"] = one_ex("one_report25", 25, 0.0)
        runs["batch_tol"] = batch_ex("batch_tol", MAX_ITERS, TOL)
        runs["one_tol"] = one_ex("one_tol", MAX_ITERS, TOL)
        runs["batch_tol"]()   # the iterations the tol form runs: the count of the fixed form beside it
        runs["one_tol"]()
        kb, k1 = int(done.max()), int(d1[0])
        assert (done == kb).all(), "the 8 windows are one group"
        runs["batch_fixed_at_stop"] = batch_ex("batch_fixed_at_stop", kb, 0.0)
        runs["one_fixed_at_stop"] = one_ex("one_fixed_at_stop", k1, 0.0)
    times = {k: [] for k in runs}
    for r in range(WARMUP + CALLS):   # the forms alternate inside one process
        for k, fn in runs.items():
            ms, wall = ev.time_ms(fn)
            if r >= WARMUP:
                times[k].append((ms, wall))
            if k in seen:
                last[k] = seen[k]()
            assert (status == 0).all()
    res = {"step": step, "lib": os.path.basename(_lib.LIB_PATH), "c2_windows": n,
           "edges_per_call": int(edges.sum()) if step == "plain" else None}
    for k, v in times.items():
        res[k] = {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
                  "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}
        res[k].update(last.get(k, {}))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (a)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window_iters.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--dry", action="store_true", help="generate the tables and stop (no GPU)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--tables", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tables)
    import bench

    c2_normal, c2_tabs = bench.c2_windows(a.windows, a.ops, a.traces, 0)
    _, c3_normal, c3_tab = bench.make_window(4242, 500, 20_000)
    print("tables:", [t.n_spans for t in c2_tabs], c3_tab.n_spans, flush=True)
    if a.dry:
        return
    steps = [("ex", None)]
    if a.parent_lib:
        steps += [("plain", None), ("plain", a.parent_lib)] * 2
    out = {"calls": CALLS, "warmup": WARMUP, "tol": TOL, "check_every": EVERY, "max_iters": MAX_ITERS, "steps": []}
    with tempfile.TemporaryDirectory() as tmp:
        tf = os.path.join(tmp, "tables.pkl")
        with open(tf, "wb") as f:
            pickle.dump((c2_normal, c2_tabs, c3_normal, c3_tab), f, protocol=pickle.HIGHEST_PROTOCOL)
        for step, libpath in steps:
            env = dict(os.environ)
            env.pop("MR_LIB_PATH", None)
            if libpath:
                env["MR_LIB_PATH"] = os.path.abspath(libpath)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step,
                   "--tables", tf]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            if p.returncode != 0:   # nothing more on the GPU after a step that failed
                print(f"step {step} ({libpath or 'this tree'}) ended with status {p.returncode}", flush=True)
                sys.exit(p.returncode)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            out["steps"].append(json.loads(line[len("RESULT "):]))
    ex = out["steps"][0]
    med = lambda k: ex[k]["event_ms_median"]   # noqa: E731
    out["b_report_cost_us"] = {"batch": (med("batch_report25") - med("batch_plain")) * 1e3,
                               "one": (med("one_report25") - med("one_plain")) * 1e3}
    out["c_tol_over_fixed"] = {"batch": med("batch_tol") / med("batch_fixed_at_stop"),
                               "one": med("one_tol") / med("one_fixed_at_stop")}
    if a.parent_lib:
        for lib in sorted({s["lib"] for s in out["steps"][1:]}):
            for k in ("batch_plain", "one_plain"):
                out[f"a_{k}_ms_{lib}"] = [s[k]["event_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "steps"}), flush=True)


if __name__ == "__main__":
    main()
