"""What one C2 span table's upload costs (mr_spans_upload: copies, the per-trace index, the layout
order and the complement form's totals / candidates / time summary), by the host's clock -- the
call returns after synchronising its stream.

One bench table (bench.c2_windows(1, 1000, 200_000, 0): 200k traces, ~2.7M rows) is uploaded
WARMUP + CALLS times, each handle closed again; prints one JSON line with the median, min and max
of the CALLS uploads in ms.  The library is MR_LIB_PATH's (another build of it) or the tree's: run
it once per library, processes alternating, to compare two builds.

    python3 scripts/upload_cost.py [--calls 15]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import bench

    _, (tab,) = bench.c2_windows(1, 1000, 200_000, 0)   # (its pool forks before the GPU is touched)
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    ms = []
    for i in range(args.warmup + args.calls):
        ctx.sync()
        t = time.perf_counter()
        dev = DeviceSpans(ctx, tab)
        ctx.sync()
        ms.append((time.perf_counter() - t) * 1e3)
        dev.close()
    ms = ms[args.warmup:]
    print(json.dumps({"what": "mr_spans_upload of one C2 table, host clock", "library": os.path.basename(_lib.LIB_PATH),
                      "rows": int(tab.n_spans), "traces": int(tab.n_traces), "calls": len(ms),
                      "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                      "ms_max": round(max(ms), 4)}))


if __name__ == "__main__":
    main()
