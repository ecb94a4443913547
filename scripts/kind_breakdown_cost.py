"""What the kind breakdown costs on one MI355X (DESIGN §3 "Kind breakdown").

The C2-shaped windows of bench.c2_windows(8, 1000, 200_000, rank=3) (8 distinct windows of one system,
the SLO of its normal period from mr_slo), each window's top list of one rank_windows call (11 ops)
plus the whole window (-1), m = 8.  Medians of 15 calls, each bracketed by HIP events on the context
stream and by the host's clock (the call ends in a read-back: the host time is what a caller waits for):

  (a) plain rank_windows and windows_latency under this tree's library and under another build of it
      (--parent-lib: the commit before), processes alternating -- their code did not change, the list
      functions only moved into a header: DESIGN §4's +-3 %;
  (b) one windows_kind_breakdown call over the 8 windows, detectors included: per call and per window;
  (c) the host form on the same windows, checked equal entry for entry: mr_detect with its state
      download, then numpy over the table's rows (the live rows' distinct (trace, pod-op) pairs, two
      64-bit sums of per-op random words per trace as the set's key, np.unique over (key, key, ops,
      span count) rows, bincounts and minima per kind, a lexsort per asked op).

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the run.
The parent process prepares the tables and never opens the GPU.

    python3 scripts/kind_breakdown_cost.py [--parent-lib PATH] [--out profiles/kind_breakdown.json]
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
N_WIN, M = 8, 8


def summary(v):
    return {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
            "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}


def host_form(np, table, state, asked, m, words):
    """windows_kind_breakdown's dict of one window from the host: state[] (mr_detect's download) and the
    table's rows."""
    P = table.n_podops
    live_rows = np.isin(state, (1, 2))[table.trace]
    key = np.unique(table.trace[live_rows].astype(np.int64) * P + table.podop[live_rows])
    tr, op = key // P, key % P
    first = np.flatnonzero(np.r_[True, tr[1:] != tr[:-1]])
    traces = tr[first]                                            # the live traces, ascending
    h1 = np.add.reduceat(words[0][op], first)
    h2 = np.add.reduceat(words[1][op], first)
    nops = np.diff(np.r_[first, tr.size]).astype(np.uint64)
    rows = np.bincount(table.trace, minlength=table.n_traces)[traces]
    w = (1.0 / rows).astype(np.float32).view(np.uint32).astype(np.uint64)
    _, inv = np.unique(np.stack([h1, h2, nops, w], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    nk = int(inv.max()) + 1
    ab = state[traces] == 2
    n_abn, n_nor = np.bincount(inv[ab], minlength=nk), np.bincount(inv[~ab], minlength=nk)
    big = np.iinfo(np.int64).max
    fa, fn = np.full(nk, big), np.full(nk, big)
    np.minimum.at(fa, inv[ab], traces[ab])
    np.minimum.at(fn, inv[~ab], traces[~ab])
    rep = np.where(n_abn > 0, fa, fn)
    pos = np.searchsorted(traces, rep)
    spans, ops = rows[pos], nops[pos].astype(np.int64)
    kind_of_pair = np.repeat(inv, np.diff(np.r_[first, tr.size]))
    out = {}
    for c in asked:
        sel = np.arange(nk) if c is None else np.unique(kind_of_pair[op == c])
        order = sel[np.lexsort((rep[sel], n_nor[sel], -n_abn[sel]))][:m]
        out[c] = (list(zip(rep[order].tolist(), n_abn[order].tolist(), n_nor[order].tolist(), spans[order].tolist(),
                           ops[order].tolist())), int(sel.size), int(n_abn[sel].sum()), int(n_nor[sel].sum()))
    return out


def child(step, tables_file):
    import numpy as np

    import bench
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows, windows_kind_breakdown, windows_latency
    from microrank_amd.preprocess_data import DeviceSpans

    with open(tables_file, "rb") as f:
        normal, abnormal = pickle.load(f)
    lib = _lib.load()
    ctx = _lib.default_context()
    a3, ok = bench.slo_from_gpu(ctx, normal)
    devs = [DeviceSpans(ctx, t) for t in abnormal]
    wins = []
    for t, d in zip(abnormal, devs):
        t0 = int(t.tstart.min())
        wins.append((d, t0, t0 + 5 * 60 * 10**9, a3, ok))
    ev = Events(lib.mr_ctx_stream(ctx.h))
    res = {"step": step, "lib": os.path.basename(_lib.LIB_PATH), "windows": len(wins)}

    def timed(fn, calls=CALLS, warmup=WARMUP):
        t = []
        for r in range(warmup + calls):
            x = ev.time_ms(fn)
            if r >= warmup:
                t.append(x)
        return summary(t)

    keep = {}
    res["plain"] = timed(lambda: keep.__setitem__("r", rank_windows(ctx, wins)))
    tops = [r[0] for r in keep["r"]]
    res["latency"] = timed(lambda: windows_latency(ctx, wins, tops))
    if step == "kinds":
        asked = [[None] + t.tolist() for t in tops]
        res["asked_per_window"] = [len(a) for a in asked]
        res["kinds"] = timed(lambda: keep.__setitem__("k", windows_kind_breakdown(ctx, wins, asked, m=M)))
        rng = np.random.default_rng(1)
        words = rng.integers(0, 1 << 63, (2, abnormal[0].n_podops), dtype=np.int64).astype(np.uint64)

        def host():
            out = []
            for t, w, a in zip(abnormal, wins, asked):
                state = np.zeros(t.n_traces, np.uint8)
                na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
                ctx.check(lib.mr_detect(ctx.h, w[0].h, w[1], w[2], _lib.ptr(a3, C.c_double), _lib.ptr(ok, C.c_uint8),
                                        _lib.ptr(state, C.c_uint8), C.byref(na), C.byref(nn), C.byref(nin)), "mr_detect")
                out.append(host_form(np, t, state, a, M, words))
            keep["h"] = out

        res["host_form"] = timed(host, calls=3, warmup=1)
        assert keep["h"] == keep["k"], "the host form and the device call disagree"
        res["host_form_equal"] = True
        whole = [k[None] for k in keep["k"]]
        res["live_kinds"] = [w[1] for w in whole]
        res["n_abnormal"] = [w[2] for w in whole]
        res["n_normal"] = [w[3] for w in whole]
        res["traces"] = [t.n_traces for t in abnormal]
        res["spans"] = [t.n_spans for t in abnormal]
    for d in devs:
        d.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so for (a)")
    ap.add_argument("--pairs", type=int, default=3, help="alternating process pairs of (a)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kind_breakdown.json"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--tables", default=None, help="keep / reuse the pickled tables at this path")
    ap.add_argument("--dry", action="store_true", help="prepare the tables and stop (no GPU)")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tables)
    import bench

    tmp = None
    tf = a.tables
    if not tf:
        tmp = tempfile.TemporaryDirectory()
        tf = os.path.join(tmp.name, "tables.pkl")
    if not os.path.exists(tf):
        normal, abnormal = bench.c2_windows(N_WIN, a.ops, a.traces, rank=3)
        with open(tf, "wb") as f:
            pickle.dump((normal, abnormal), f, protocol=4)
        print("tables:", normal.n_traces, [t.n_traces for t in abnormal], "traces", flush=True)
    if a.dry:
        return
    steps = [("kinds", None)]
    if a.parent_lib:
        steps += [("plain", None), ("plain", a.parent_lib)] * a.pairs
    out = {"calls": CALLS, "warmup": WARMUP, "windows": N_WIN, "m": M, "steps": []}
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
    k = out["steps"][0]
    out["b_kinds_ms_per_call"] = k["kinds"]["host_ms_median"]
    out["b_kinds_event_ms_per_call"] = k["kinds"]["event_ms_median"]
    out["b_kinds_ms_per_window"] = k["kinds"]["host_ms_median"] / N_WIN
    out["c_host_form_ms_per_window"] = k["host_form"]["host_ms_median"] / N_WIN
    out["c_host_form_over_call"] = k["host_form"]["host_ms_median"] / k["kinds"]["host_ms_median"]
    if a.parent_lib:
        for what in ("plain", "latency"):
            med = {}
            for lib in sorted({s["lib"] for s in out["steps"][1:]}):
                v = [s[what]["event_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
                out[f"a_{what}_event_ms_{lib}"] = v
                out[f"a_{what}_host_ms_{lib}"] = [s[what]["host_ms_median"] for s in out["steps"][1:] if s["lib"] == lib]
                med[lib] = statistics.median(v)   # (the ratio: by HIP events)
            libs = sorted(med)
            if len(libs) == 2:
                this = [x for x in libs if x == "libmicrorank_hip.so"]
                if this:
                    other = [x for x in libs if x != this[0]][0]
                    out[f"a_{what}_this_over_parent"] = med[this[0]] / med[other]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "steps"}), flush=True)
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
