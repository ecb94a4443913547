"""What the call evidence costs on one MI355X (DESIGN §3 "Call evidence").

The C2 bench tables: bench.c2_window_stream(N, 1000, 200_000, rank=0), N = 256 distinct windows of one
system, each its own span table resident in HBM, the SLO of the normal period from mr_slo -- the windows
of bench.py's default line.  After a warm-up, medians of CALLS calls, each bracketed by HIP events on the
context stream and by the host's clock (every call ends in a read-back: the host time is what a caller
waits for):

  (a) one ranking step: rank_windows over the N windows (one mr_windows_batch_ex call);
  (b) one windows_kind_breakdown call over the N windows: the whole window plus each top list, m = 8;
  (c) one windows_call_edges call over the N windows: each top list, m = 8;
  (d) mr_copy_peak, and the bytes the count pass of (c) reads per window under the assumption that every
      trace is in the window's partition (a C2 window spans its table): 5 B per row (its trace code and
      that trace's state byte) and, for a row with a parent, 49 B more -- parent 8, id_off 16, duration 8,
      pod-op 4, id_rows 4, the parent row's trace 4, state 1 and pod-op 4 (the binary search in the edge
      dictionary stays in cache and is not counted).

  (e) one windows_latency call (q = 0.5 and 0.99, self time) and one windows_timeline call (30 buckets, self
      time) over the N windows: each top list;
  (f) one windows_replicas call over the N windows: each top list, m = 8, self time.

The GPU work runs in one child process under `timeout`; the parent never opens the GPU.

    python3 scripts/call_edges_cost.py [--windows 256] [--out profiles/call_edges.json]

--parent-lib PATH (another build of libmicrorank_hip.so: the commit before) answers "did the code get slower"
for a change that is meant to leave the timings alone: four child processes, the library chosen by
MR_LIB_PATH, alternating parent, this tree, parent, this tree, each under `timeout`; the first one that fails
ends the run.  Per timed entry the mean of this tree's two medians against the larger of the parent's two
times 1.03 (DESIGN §4's box-to-box spread); the parent's own two medians say how far one build moves between
processes.  The result goes to profiles/evidence_front.json.

--parent-tree DIR (a checkout of the commit before) asks the same of a change to the Python side: the four
children alternate DIR's package and this tree's, all four over this tree's library, and the bar applies to
the medians by HIP events and to those by the host's clock.  The result goes to profiles/evidence_python.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from converge_cost import Events  # noqa: E402  (scripts/ is sys.path[0])

CALLS, WARMUP, M = 7, 2, 8
TIMED = ("ranking_step", "kind_breakdown", "call_edges", "latency", "timeline", "replicas")
SPREAD = 1.03


def summary(v):
    return {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
            "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}


def child(a):
    import ctypes as C

    if a.tree:   # (the package and bench.py of another checkout, ahead of this one's)
        sys.path.insert(0, os.path.abspath(a.tree))
    import bench
    from microrank_amd import _lib
    from microrank_amd.online_rca import (rank_windows, windows_call_edges, windows_kind_breakdown, windows_latency,
                                          windows_replicas, windows_timeline)
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(a.tree or REPO), "microrank_amd")
    from microrank_amd.preprocess_data import DeviceSpans

    tabs = bench.c2_window_stream(a.windows, a.ops, a.traces, 0)   # (the generators fork before the GPU is touched)
    lib = _lib.load()
    ctx = _lib.default_context()
    a3, ok = bench.slo_from_gpu(ctx, next(tabs))
    wins, rows, with_parent = [], [], []
    for t in tabs:
        t0 = int(t.tstart.min())
        rows.append(int(t.n_spans))
        with_parent.append(int((t.parent >= 0).sum()))
        d = DeviceSpans(ctx, t)
        d.table = None   # (the host columns are slab views the next tables overwrite)
        wins.append((d, t0, t0 + 5 * 60 * 10**9, a3, ok))
    ev = Events(lib.mr_ctx_stream(ctx.h))
    res = {"lib": a.child, "windows": len(wins), "ops": a.ops, "traces": a.traces, "calls": CALLS, "warmup": WARMUP, "m": M,
           "rows_per_window": [min(rows), statistics.median(rows), max(rows)]}

    def timed(fn):
        t = []
        for r in range(WARMUP + CALLS):
            x = ev.time_ms(fn)
            if r >= WARMUP:
                t.append(x)
        return summary(t)

    keep = {}
    res["ranking_step"] = timed(lambda: keep.__setitem__("r", rank_windows(ctx, wins)))
    tops = [r[0] for r in keep["r"]]
    res["asked_per_window"] = [min(len(t) for t in tops), max(len(t) for t in tops)]
    res["kind_breakdown"] = timed(lambda: windows_kind_breakdown(ctx, wins, [[None] + t.tolist() for t in tops], m=M))
    res["call_edges"] = timed(lambda: keep.__setitem__("c", windows_call_edges(ctx, wins, tops, m=M)))
    res["latency"] = timed(lambda: windows_latency(ctx, wins, tops, q=(0.5, 0.99), what="self"))
    res["timeline"] = timed(lambda: windows_timeline(ctx, wins, tops, buckets=30, what="self"))
    res["replicas"] = timed(lambda: windows_replicas(ctx, wins, tops, m=M, what="self"))
    listed = [sum(len(side[0]) for v in w.values() for side in v) for w in keep["c"]]
    res["listed_edges_per_window"] = [min(listed), max(listed)]
    res["calls_per_window_abn_nor"] = [[sum(v[1][2][k] for v in w.values()) for k in (0, 1)] for w in keep["c"][:4]]
    g = C.c_double()
    ctx.check(lib.mr_copy_peak(ctx.h, 1 << 30, 5, C.byref(g)), "mr_copy_peak")
    res["copy_peak_gbs"] = g.value
    byt = [5 * s + 49 * p for s, p in zip(rows, with_parent)]
    res["count_pass_bytes_per_window"] = [min(byt), statistics.median(byt), max(byt)]
    res["count_pass_bytes_per_call"] = sum(byt)
    res["call_fraction_of_copy_peak"] = sum(byt) / (res["call_edges"]["event_ms_median"] * 1e-3) / (g.value * 1e9)
    for w in wins:
        w[0].close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(a, role, libpath, tree=None):
    """One child process under `timeout`: its RESULT line, or None when the step failed."""
    env = dict(os.environ)
    env.pop("MR_LIB_PATH", None)
    if libpath:
        env["MR_LIB_PATH"] = os.path.abspath(libpath)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", role,
           "--windows", str(a.windows), "--ops", str(a.ops), "--traces", str(a.traces)]
    cmd += ["--tree", tree] if tree else []
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"the GPU step ({role}) failed (exit status {p.returncode})", flush=True)
        return None
    return json.loads(line[-1][len("RESULT "):])


def compare(steps, clock="event_ms_median"):
    """Per timed entry: the four medians by ``clock`` and whether this tree keeps the parent's time."""
    out = {}
    for what in TIMED:
        old = [s[what][clock] for s in steps if s["lib"] == "parent"]
        new = [s[what][clock] for s in steps if s["lib"] == "new"]
        bar = max(old) * SPREAD
        out[what] = {"parent_ms": old, "new_ms": new, "new_mean_ms": statistics.mean(new), "bar_ms": bar,
                     "within_bar": statistics.mean(new) <= bar, "parent_spread": max(old) / min(old),
                     "parent_moved_more_than_bar": max(old) / min(old) > SPREAD}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None, help="another build of libmicrorank_hip.so: compare against it")
    ap.add_argument("--parent-tree", default=None,
                    help="a checkout of the commit before: compare its Python package against this one's")
    ap.add_argument("--tree", default=None, help="(internal) the checkout a child takes the package from")
    ap.add_argument("--out", default=None, help="default: profiles/call_edges.json, evidence_front.json with --parent-lib, "
                                                "evidence_python.json with --parent-tree")
    ap.add_argument("--step-timeout", type=int, default=840)
    ap.add_argument("--child", default=None, help="(internal) run the GPU step; the value names the library")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.parent_lib and a.parent_tree:
        ap.error("--parent-lib and --parent-tree are two questions: ask one")
    out = a.out or os.path.join(REPO, "profiles", "evidence_python.json" if a.parent_tree else
                                "evidence_front.json" if a.parent_lib else "call_edges.json")
    if a.parent_lib or a.parent_tree:
        steps = []
        own = os.path.join(REPO, "microrank_amd", "libmicrorank_hip.so") if a.parent_tree else None   # (one library for all)
        for role in ("parent", "new", "parent", "new"):
            old = role == "parent"
            r = run_child(a, role, own or (a.parent_lib if old else None), a.parent_tree if old else None)
            if r is None:   # nothing more on the GPU after a step that failed
                sys.exit(1)
            print(json.dumps({k: r[k]["event_ms_median"] for k in TIMED} | {"lib": role}), flush=True)
            steps.append(r)
        res = {"windows": a.windows, "ops": a.ops, "traces": a.traces, "calls": CALLS, "warmup": WARMUP, "m": M,
               "spread": SPREAD, "entries": compare(steps), "steps": steps}
        shown = res["entries"]
        if a.parent_tree:   # (host code changed: the host's clock is held to the bar too)
            res["entries_host_clock"] = compare(steps, "host_ms_median")
            res["all_within_bar"] = all(e["within_bar"] for k in ("entries", "entries_host_clock") for e in res[k].values())
            shown = {k: res[k] for k in ("entries", "entries_host_clock", "all_within_bar")}
    else:
        res = shown = run_child(a, "new", None)
        if res is None:
            sys.exit(1)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(shown, indent=1))


if __name__ == "__main__":
    main()
