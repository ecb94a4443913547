"""What the replica evidence costs on one MI355X (DESIGN §3 "Replica evidence").

Two workloads, after a warm-up medians of CALLS calls, each bracketed by HIP events on the context stream and
by the host's clock (every call ends in a read-back: the host time is what a caller waits for); every entry
is measured twice, the entries alternating:

  (a) the C2 bench tables: bench.c2_window_stream(N, 1000, 200_000, rank=0), N = 256 distinct windows of one
      system, each its own span table resident in HBM, the SLO of the normal period from mr_slo, each
      window's top ops of one rank_windows call.  The C2 generator has ONE pod per service, so every asked
      op is its service-op's only replica: the row pass at its cheapest selection;
  (b) one multi-pod table, synth.window_pair(40, 100_000, 3, pods=3) (100k traces, 1.86M rows, 40 service-ops
      of 3 replicas each), asked as PODS_WINDOWS windows over its whole time range with the 11 pod-ops that have
      the most rows on abnormal traces.

Per workload: one windows_replicas call (m = 8) for self time and for duration, the same call with nothing
asked (the detectors, the zeroing and the read-back alone), and the yardstick in the same process on the same
windows: one windows_timeline call (30 buckets, same what).  The Python entries build their answers (a dict per
asked op); `*_raw` are the two C entries alone (tests/*_cases.call).  profiles/replicas.json also keeps the
`*_sv_first` entries of the run that decided the row pass's read order: the variant that reads the service-op
before the trace's state, behind a knob that the kernel no longer has.
Then mr_copy_peak and the bytes the row pass reads per call under the assumption that every trace is in the
window's partition: 9 B per row (trace code, state byte, service-op) and, for a row of an asked service-op,
16 B more (pod-op, its rank, the duration), 32 B for self time (span, csum).

The GPU work runs in one child process under `timeout`; the parent never opens the GPU.

    python3 scripts/replicas_cost.py [--windows 256] [--out profiles/replicas.json]
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

CALLS, WARMUP, M, BUCKETS, PODS_WINDOWS = 7, 2, 8, 30, 32


def summary(v):
    return {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
            "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}


def measure(ev, ctx, wins, tops):
    """Every entry twice, alternating: {entry: [summary, summary]}."""
    from microrank_amd.online_rca import windows_replicas, windows_timeline

    import replica_cases as rc
    import timeline_cases as tc

    def timed(fn):
        t = []
        for r in range(WARMUP + CALLS):
            x = ev.time_ms(fn)
            if r >= WARMUP:
                t.append(x)
        return summary(t)

    entries = {}
    for what in ("self", "duration"):
        entries[f"timeline_{what}"] = lambda what=what: windows_timeline(ctx, wins, tops, buckets=BUCKETS, what=what)
        entries[f"replicas_{what}"] = lambda what=what: windows_replicas(ctx, wins, tops, m=M, what=what)
    entries["replicas_nothing_asked"] = lambda: windows_replicas(ctx, wins, [[] for _ in wins], m=M)
    # the C entries alone (tests/*_cases.call: the raw call into garbage-filled buffers, no Python answer built)
    kmax = max(len(t) for t in tops)
    b0, bw = [w[1] for w in wins], [(w[2] - w[1]) // BUCKETS + 1 for w in wins]
    entries["timeline_self_raw"] = lambda: tc.call(ctx, wins, tops, kmax, BUCKETS, "self", b0, bw)
    entries["replicas_self_raw"] = lambda: rc.call(ctx, wins, tops, kmax, M, "self")
    out = {k: [] for k in entries}
    for _ in range(2):
        for k, fn in entries.items():
            out[k].append(timed(fn))
    return out


def child(a):
    import ctypes as C

    import bench
    from microrank_amd import _lib, synth
    from microrank_amd.online_rca import rank_windows, windows_replicas
    from microrank_amd.preprocess_data import DeviceSpans

    import latency_cases as lc
    import replica_cases as rc

    tabs = bench.c2_window_stream(a.windows, a.ops, a.traces, 0)   # (the generators fork before the GPU is touched)
    lib = _lib.load()
    ctx = _lib.default_context()
    a3, ok = bench.slo_from_gpu(ctx, next(tabs))
    wins, rows = [], []
    for t in tabs:
        t0 = int(t.tstart.min())
        rows.append(int(t.n_spans))
        d = DeviceSpans(ctx, t)
        d.table = None   # (the host columns are slab views the next tables overwrite)
        wins.append((d, t0, t0 + 5 * 60 * 10**9, a3, ok))
        if len(wins) % 32 == 0:
            print(f"{len(wins)} tables resident", flush=True)
    ev = Events(lib.mr_ctx_stream(ctx.h))
    res = {"windows": len(wins), "ops": a.ops, "traces": a.traces, "calls": CALLS, "warmup": WARMUP, "m": M,
           "buckets": BUCKETS, "rows_per_window": [min(rows), statistics.median(rows), max(rows)]}

    def selected(rp):   # the rows on the lists' service-ops, each service-op once (its totals: the selected rows)
        return [sum(sum(t[:2]) for t in {r["total"] + tuple(e[0] for e in r["entries"]) for r in w.values()}) for w in rp]

    def bytes_of(rows, sel):
        return {"duration": sum(9 * s + 16 * x for s, x in zip(rows, sel)), "self": sum(9 * s + 32 * x for s, x in zip(rows, sel))}

    def report(tag, wins, tops, rows):
        r = measure(ev, ctx, wins, tops)
        rp = windows_replicas(ctx, wins, tops, m=M)
        sel = selected(rp)
        res[tag] = {"entries": r, "asked_per_window": [min(len(t) for t in tops), max(len(t) for t in tops)],
                    "replicas_per_asked_op": [min(v["all"] for w in rp for v in w.values()),
                                              max(v["all"] for w in rp for v in w.values())],
                    "selected_rows_per_window": [min(sel), statistics.median(sel), max(sel)],
                    "row_pass_bytes_per_call": bytes_of(rows, sel)}
        print(tag, json.dumps({k: [x["event_ms_median"] for x in v] for k, v in r.items()}), flush=True)

    tops = [r[0] for r in rank_windows(ctx, wins)]
    report("c2", wins, tops, rows)
    for w in wins:
        w[0].close()
    _, normal, abnormal = synth.window_pair(40, 100_000, 3, pods=3)
    pa3, pok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
    dev = DeviceSpans(ctx, abnormal)
    pwins = [(dev, t0, t1, pa3, pok)] * PODS_WINDOWS
    ptops = [rc.top_by_abnormal_rows(abnormal, state)] * PODS_WINDOWS   # (the 11 pod-ops with the most abnormal rows)
    res["pods3_table"] = {"rows": int(abnormal.n_spans), "pod_ops": int(abnormal.n_podops), "service_ops": int(abnormal.n_svcops),
                          "windows": PODS_WINDOWS}
    report("pods3", pwins, ptops, [int(abnormal.n_spans)] * PODS_WINDOWS)
    dev.close()
    g = C.c_double()
    ctx.check(lib.mr_copy_peak(ctx.h, 1 << 30, 5, C.byref(g)), "mr_copy_peak")
    res["copy_peak_gbs"] = g.value
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--ops", type=int, default=1000)
    ap.add_argument("--traces", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replicas.json"))
    ap.add_argument("--step-timeout", type=int, default=840)
    ap.add_argument("--child", action="store_true", help="(internal) run the GPU step")
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--windows", str(a.windows), "--ops", str(a.ops), "--traces", str(a.traces)]
    line = []
    with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True) as p:
        for ln in p.stdout:   # (the child's progress lines as they come)
            if ln.startswith("RESULT "):
                line.append(ln)
            else:
                print(ln, end="", flush=True)
    if p.returncode != 0 or not line:
        print(f"the GPU step failed (exit status {p.returncode})", flush=True)
        sys.exit(1)
    res = json.loads(line[-1][len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("c2", "pods3")}, indent=1))


if __name__ == "__main__":
    main()
