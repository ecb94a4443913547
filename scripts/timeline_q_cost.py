"""What the timeline's quantiles per bucket cost on one MI355X (DESIGN §3 "Timeline evidence").

One call over WINDOWS C2 windows (bench.c2_window_stream(8, 1000, 200_000, rank=0): 8 distinct windows of one
system, each its own span table resident in HBM, the SLO of the normal period from mr_slo), each asked its
ranking's top list (up to 11 ops) and -1, B = 30 buckets, q = (0.5, 0.99), self time.  After a warm-up medians of
CALLS calls, each bracketed by HIP events on the context stream and by the host's clock (every call ends in a
read-back: the host time is what a caller waits for).  The entries are the raw C calls of tests/*_cases.py.

  1. plain mr_windows_timeline, this library against another build of it (--parent-lib: the parent commit's
     libmicrorank_hip.so, loaded through MR_LIB_PATH): processes alternating, two of each.  The entry promises
     "unchanged"; `plain_unchanged` says whether every median of this library lies within the other's min-max
     spread widened by DESIGN §4's +-3 % box-to-box figure.
  2. mr_windows_timeline_q, against (a) the plain timeline call plus one mr_windows_latency call on the same
     windows and ops -- the nearest existing work: it also makes two row passes and a sort -- and (b) the host
     form: mr_detect's state downloaded per window, then the numpy oracle of tests/timeline_q_cases.py.

Every GPU step runs in a child process of its own under `timeout`; the parent never opens the GPU.

    python3 scripts/timeline_q_cost.py --parent-lib /path/to/parent/libmicrorank_hip.so [--out profiles/timeline_q.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from converge_cost import Events  # noqa: E402  (scripts/ is sys.path[0])

WINDOWS, OPS, TRACES, CALLS, WARMUP, BUCKETS, Q, HOST_CALLS = 8, 1000, 200_000, 15, 3, 30, (0.5, 0.99), 3
BOX = 0.03   # the same binary differs by up to +-3 % from box to box


def summary(v):
    return {"event_ms_median": statistics.median(m for m, _ in v), "event_ms_min": min(m for m, _ in v),
            "event_ms_max": max(m for m, _ in v), "host_ms_median": statistics.median(w for _, w in v)}


def child(a):
    import ctypes as C

    import numpy as np

    import bench
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.online_rca import rank_windows
    from microrank_amd.preprocess_data import DeviceSpans

    import latency_cases as lc
    import timeline_cases as tc

    tabs = bench.c2_window_stream(WINDOWS, OPS, TRACES, 0)   # (the generators fork before the GPU is touched)
    lib = _lib.load()
    ctx = _lib.default_context()
    a3, ok = bench.slo_from_gpu(ctx, next(tabs))
    wins, host = [], []
    for t in tabs:
        t0 = int(t.tstart.min())
        d = DeviceSpans(ctx, t)
        host.append(bench.own_table(t) if a.child == "quantiles" else None)   # (the host form reads the columns)
        d.table = None
        wins.append((d, t0, t0 + 5 * 60 * 10**9, a3, ok))
    tops = [r[0].tolist() + [-1] for r in rank_windows(ctx, wins)]
    kmax = max(len(t) for t in tops)
    b0, bw = [w[1] for w in wins], [(w[2] - w[1]) // BUCKETS + 1 for w in wins]
    ev = Events(lib.mr_ctx_stream(ctx.h))

    def timed(fn, calls=CALLS, warmup=WARMUP):
        t = []
        for r in range(warmup + calls):
            x = ev.time_ms(fn)
            if r >= warmup:
                t.append(x)
        return summary(t)

    res = {"lib": os.path.basename(_lib.LIB_PATH), "rows_per_window": [int(h.n_spans) for h in host if h is not None],
           "asked_per_window": [len(t) for t in tops]}
    res["timeline_plain"] = timed(lambda: tc.call(ctx, wins, tops, kmax, BUCKETS, "self", b0, bw))
    if a.child == "quantiles":
        import timeline_q_cases as tq

        def latency():
            n = len(wins)
            only = [[c for c in t if c >= 0] for t in tops]
            spans = (_lib.P * n)(*[w[0].h for w in wins])
            t0, t1 = np.array([w[1] for w in wins], np.int64), np.array([w[2] for w in wins], np.int64)
            pa3 = (C.c_void_p * n)(*[a3.ctypes.data] * n)
            pok = (C.c_void_p * n)(*[ok.ctypes.data] * n)
            cod = np.zeros((n, kmax), np.int32)
            for i, o in enumerate(only):
                cod[i, :len(o)] = o
            n_ops = np.array([len(o) for o in only], np.int32)
            qv = np.array(Q, np.float64)
            out, cnt = np.zeros((n, kmax, 2, qv.size)), np.zeros((n, kmax, 2), np.int64)
            status = np.zeros(n, np.int32)
            ctx.check(lib.mr_windows_latency(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), pa3, pok,
                                             ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), kmax, lc.WHAT["self"],
                                             ptr(qv, C.c_double), qv.size, 0, ptr(out, C.c_double), ptr(cnt, C.c_int64),
                                             ptr(status, C.c_int32)), "mr_windows_latency")
            return out

        def pair():
            tc.call(ctx, wins, tops, kmax, BUCKETS, "self", b0, bw)
            latency()

        def quantiles():
            return tq.call(ctx, wins, tops, kmax, BUCKETS, "self", b0, bw, Q, "linear")

        def host_form():
            got = []
            for (d, w0, w1, _, _), t, asked in zip(wins, host, tops):
                state = np.zeros(t.n_traces, np.uint8)
                na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
                ctx.check(lib.mr_detect(ctx.h, d.h, w0, w1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), ptr(state, C.c_uint8),
                                        C.byref(na), C.byref(nn), C.byref(nin)), "mr_detect")
                got.append(tq.quantile_oracle(t, state, asked, kmax, BUCKETS, "self", w0, (w1 - w0) // BUCKETS + 1, Q,
                                              "linear", w0, w1)[0])
            return got

        for _ in range(2):   # every entry twice, alternating
            for name, fn in (("timeline_q", quantiles), ("timeline_plus_latency", pair), ("latency", latency)):
                res.setdefault(name, []).append(timed(fn))
        t = time.perf_counter()
        want = host_form()
        first = (time.perf_counter() - t) * 1e3
        res["host_form"] = {"host_ms": [first] + [ev.time_ms(host_form)[1] for _ in range(HOST_CALLS - 1)]}
        res["host_form"]["host_ms_median"] = statistics.median(res["host_form"]["host_ms"])
        _, out, _ = quantiles()
        res["equals_host_form"] = all(lc.hexes(o.q) == lc.hexes(w) for o, w in zip(out, want))
        res["classes_with_values"] = int(sum((o.cnt > 0).sum() for o in out))
        res["selected_values"] = int(sum(o.cnt.sum() for o in out))
    print("RESULT " + json.dumps(res), flush=True)


def run_child(a, kind, lib_path):
    env = dict(os.environ)
    env.pop("MR_LIB_PATH", None)
    if lib_path:
        env["MR_LIB_PATH"] = lib_path
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", kind]
    line = []
    with subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env) as p:
        for ln in p.stdout:
            if ln.startswith("RESULT "):
                line.append(ln)
            else:
                print(ln, end="", flush=True)
    if p.returncode != 0 or not line:
        print(f"the GPU step {kind} failed (exit status {p.returncode})", flush=True)
        sys.exit(1)   # (nothing more is started on the GPU)
    return json.loads(line[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmicrorank_hip.so (measurement 1)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "timeline_q.json"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--child", default=None, help="(internal) run a GPU step: plain | quantiles")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"windows": WINDOWS, "ops": OPS, "traces": TRACES, "calls": CALLS, "warmup": WARMUP, "buckets": BUCKETS,
           "q": list(Q), "box_to_box": BOX}
    if a.parent_lib:
        runs = {"parent": [], "this": []}
        for _ in range(2):
            for who, path in (("this", None), ("parent", os.path.abspath(a.parent_lib))):
                runs[who].append(run_child(a, "plain", path)["timeline_plain"])
                print(who, json.dumps(runs[who][-1]), flush=True)
        lo = min(r["event_ms_min"] for r in runs["parent"]) * (1 - BOX)
        hi = max(r["event_ms_max"] for r in runs["parent"]) * (1 + BOX)
        res["plain"] = dict(runs, allowed_ms=[lo, hi],
                            plain_unchanged=all(lo <= r["event_ms_median"] <= hi for r in runs["this"]))
    res["quantiles"] = run_child(a, "quantiles", None)
    q = [r["event_ms_median"] for r in res["quantiles"]["timeline_q"]]
    pair = res["quantiles"]["timeline_plus_latency"]
    res["q_over_pair"] = statistics.mean(q) / statistics.mean(r["event_ms_median"] for r in pair)
    res["pair_spread_ms"] = [min(r["event_ms_min"] for r in pair), max(r["event_ms_max"] for r in pair)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
