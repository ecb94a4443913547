"""What a window batch's exemplars cost on one MI355X (DESIGN §3 "K2 exemplars", window batches).

The C2-shaped window of bench.make_window (1000 ops, 200k traces; the SLO of its normal period from
mr_slo), 64 such windows in one rank_windows call.  Medians of 15 calls, each bracketed by HIP events
on the context stream and by the host's clock (the call ends in a read-back: the host time is what a
caller waits for):

  (a) plain rank_windows under this tree's library and under another build of it (--parent-lib: the
      commit before), processes alternating -- "the plain path did not move" (DESIGN §4's +-3 %);
  (b) rank_windows(exemplars=5) against plain, same process: the added time per call and per window,
      and the Python side of it alone (the rows built from arrays of the call's shape);
  (c) the same windows through the composed form, rca_window(..., exemplars=5), a window at a time
      (--composed-windows of them: the windows are alike);
  (d) the byte floor of the selection: 2 B per id of the tiles + 8 B per trace of the abnormal
      traces' graph, per window, over mr_copy_peak's measured rate.

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the run.
The parent process prepares the tables and never opens the GPU.

    python3 scripts/window_exemplar_cost.py [--parent-lib PATH] [--out profiles/window_exemplars.json]
    python3 scripts/window_exemplar_cost.py --child trace ...   (the loop rocprofv3 --kernel-trace wraps)
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

CALLS, WARMUP = 15, 3
N_WIN, M = 64, 5


def summary(v):
    return {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
            "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}


def child(step, tables_file, composed_windows):
    import numpy as np

    import bench
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows, rca_window
    from microrank_amd.preprocess_data import DeviceSpans

    with open(tables_file, "rb") as f:
        normal, abnormal = pickle.load(f)
    lib = _lib.load()
    ctx = _lib.default_context()
    a3, ok = bench.slo_from_gpu(ctx, normal)
    dev = DeviceSpans(ctx, abnormal)
    t0 = int(abnormal.tstart.min())
    t1 = t0 + 5 * 60 * 10**9
    wins = [(dev, t0, t1, a3, ok)] * N_WIN
    ev = Events(lib.mr_ctx_stream(ctx.h))
    res = {"step": step, "lib": os.path.basename(_lib.LIB_PATH), "windows": N_WIN}

    def timed(fn, calls=CALLS, warmup=WARMUP):
        t = []
        for r in range(warmup + calls):
            x = ev.time_ms(fn)
            if r >= warmup:
                t.append(x)
        return summary(t)

    if step == "plain":
        res["plain"] = timed(lambda: rank_windows(ctx, wins))
    elif step == "trace":   # (under rocprofv3 --kernel-trace --stats: the kernels of the exemplar tail)
        for _ in range(WARMUP + CALLS):
            rank_windows(ctx, wins, exemplars=M)
    else:
        keep = {}
        res["plain"] = timed(lambda: keep.__setitem__("p", rank_windows(ctx, wins)))
        res["exemplars"] = timed(lambda: keep.__setitem__("e", rank_windows(ctx, wins, exemplars=M)))
        p, e = keep["p"][0], keep["e"][0]
        assert p[0].tobytes() == e[0].tobytes() and p[1].tobytes() == e[1].tobytes() and len(e[6]) == len(e[0])
        assert all(len(v) <= M for v in e[6].values()) and any(e[6].values())
        # the Python side of the keyword alone: the rows of arrays shaped as this call's
        from microrank_amd.online_rca import _exemplar_rows

        k = 11
        fake = (np.arange(N_WIN * k, dtype=np.int32), np.full(N_WIN, k, np.int32), np.zeros(N_WIN * k * M, np.int32),
                np.ones(N_WIN * k * M), np.full(N_WIN * k, M, np.int32))
        res["python_rows"] = timed(lambda: _exemplar_rows(N_WIN, k, M, *fake))
        # rca_window takes the SLO by service-op name as [mean, std]: a3 = mean + 3 * 0
        slo = {n: [float(a3[i]), 0.0] for i, n in enumerate(abnormal.svcop_names) if ok[i]}

        def composed():
            for _ in range(composed_windows):
                keep["c"] = rca_window(None, t0, t1, slo, ctx=ctx, table=abnormal, dev=dev, exemplars=M)

        res["composed"] = timed(composed, calls=5, warmup=1)
        res["composed_windows"] = composed_windows
        # the graph the selection reads: the detector's abnormal traces
        state = np.zeros(abnormal.n_traces, np.uint8)
        na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
        ctx.check(lib.mr_detect(ctx.h, dev.h, t0, t1, _lib.ptr(a3, C.c_double), _lib.ptr(ok, C.c_uint8),
                                _lib.ptr(state, C.c_uint8), C.byref(na), C.byref(nn), C.byref(nin)), "mr_detect")
        sel = state == 2
        pairs = np.unique(abnormal.trace[sel[abnormal.trace]].astype(np.int64) * abnormal.n_podops +
                          abnormal.podop[sel[abnormal.trace]])
        T, nnz = int(sel.sum()), int(pairs.size)
        gbs = C.c_double(0.0)
        ctx.check(lib.mr_copy_peak(ctx.h, 256 << 20, 5, C.byref(gbs)), "mr_copy_peak")
        floor_bytes = 2 * nnz + 8 * T
        res.update(n_abnormal=int(na.value), n_normal=int(nn.value), graph_T=T, graph_nnz=nnz, copy_peak_gbs=gbs.value,
                   floor_bytes_per_window=floor_bytes, floor_us_per_window=floor_bytes / (gbs.value * 1e3))
    dev.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (a)")
    ap.add_argument("--pairs", type=int, default=3, help="alternating process pairs of (a)")
    ap.add_argument("--composed-windows", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window_exemplars.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--tables", default=None, help="keep / reuse the pickled tables at this path")
    ap.add_argument("--dry", action="store_true", help="prepare the tables and stop (no GPU)")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tables, a.composed_windows)
    import bench

    tmp = None
    tf = a.tables
    if not tf:
        tmp = tempfile.TemporaryDirectory()
        tf = os.path.join(tmp.name, "tables.pkl")
    if not os.path.exists(tf):
        _, normal, abnormal = bench.make_window(a.seed, a.ops, a.traces)
        with open(tf, "wb") as f:
            pickle.dump((normal, abnormal), f)
        print("tables:", normal.n_traces, abnormal.n_traces, "traces", flush=True)
    if a.dry:
        return
    steps = [("exemplars", None)]
    if a.parent_lib:
        steps += [("plain", None), ("plain", a.parent_lib)] * a.pairs
    out = {"calls": CALLS, "warmup": WARMUP, "windows": N_WIN, "m": M, "steps": []}
    for step, libpath in steps:
        env = dict(os.environ)
        env.pop("MR_LIB_PATH", None)
        if libpath:
            env["MR_LIB_PATH"] = os.path.abspath(libpath)
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step,
               "--tables", tf, "--composed-windows", str(a.composed_windows)]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:   # nothing more on the GPU after a step that failed
            print(f"step {step} ({libpath or 'this tree'}) ended with status {p.returncode}", flush=True)
            sys.exit(p.returncode)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out["steps"].append(json.loads(line[len("RESULT "):]))
    ex = out["steps"][0]
    plain, with_ex = ex["plain"]["host_ms_median"], ex["exemplars"]["host_ms_median"]
    comp = ex["composed"]["host_ms_median"] / ex["composed_windows"]
    out["b_plain_ms_per_call"] = plain
    out["b_exemplars_ms_per_call"] = with_ex
    out["b_added_ms_per_call"] = with_ex - plain
    out["b_added_us_per_window"] = (with_ex - plain) * 1e3 / N_WIN
    out["b_python_rows_ms_per_call"] = ex["python_rows"]["host_ms_median"]
    out["c_composed_ms_per_window"] = comp
    out["c_batch_exemplars_ms_per_window"] = with_ex / N_WIN
    out["c_composed_over_batch"] = comp / (with_ex / N_WIN)
    out["d_floor_us_per_window"] = ex["floor_us_per_window"]
    if a.parent_lib:
        for lib in sorted({s["lib"] for s in out["steps"][1:]}):
            out[f"a_plain_host_ms_{lib}"] = [s["plain"]["host_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "steps"}), flush=True)
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
