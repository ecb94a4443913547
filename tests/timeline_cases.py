"""Helpers of the timeline-evidence tests (mr_windows_timeline, csrc/mr_timeline.hip): the numpy oracle --
exactly the semantics of include/microrank_hip.h, from the span table's rows and a detector partition
(oracle.detect's lists as mr_detect's state[]) -- and the case builders.  Everything cached here is
shared between tests and read-only."""
import ctypes as C
import functools
import types

import numpy as np

import kind_breakdown_cases as kb
import latency_cases as lc
from kind_breakdown_cases import BOUNDARY_SIZES, K_TOP, WINDOWS   # noqa: F401 -- the tests' shared figures

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIG = 1 << 62
BUCKETS = (1, 7, 30, 512)
WHATS = ("duration", "self")
NAMES = WINDOWS + ("fault",)


def wrap(v):
    """A Python int as the int64 it wraps to."""
    return (int(v) + (1 << 63)) % (1 << 64) - (1 << 63)


# ---------------------------------------------------------------------------------- the oracle
def bucket_of(ts, b0, bw, B):
    """The bucket of a start (Python ints): B for "before", B + 1 for "after"."""
    ts, b0, bw = int(ts), int(b0), int(bw)
    if ts < b0:
        return B
    b = ((ts - b0) % (1 << 64)) // bw   # (uint64)ts - (uint64)b0: exact, since ts >= b0
    return B + 1 if b >= B else b


def trace_times(table):
    """(tstart, tend) per trace code, from the trace's first row (the times are trace-level); 0 for a trace
    without rows."""
    nt = table.n_traces
    first = np.full(nt, -1, np.int64)
    first[table.trace[::-1]] = np.arange(table.n_spans - 1, -1, -1)
    has = first >= 0
    ts, te = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
    ts[has], te[has] = table.tstart[first[has]], table.tend[first[has]]
    return ts, te


def _hist(bk, side, val, B):
    """cnt / sum / max [B, 2] and out [2, 2] of the selected (bucket, side, value) triples."""
    cnt, tot = np.zeros((B + 2, 2), np.int64), np.zeros((B + 2, 2), np.int64)
    mx = np.full((B + 2, 2), I64_MIN, np.int64)
    np.add.at(cnt, (bk, side), 1)
    with np.errstate(over="ignore"):
        np.add.at(tot, (bk, side), val)   # (int64: wraps)
    np.maximum.at(mx, (bk, side), val)
    mx[cnt == 0] = 0
    return cnt[:B], tot[:B], mx[:B], np.ascontiguousarray(cnt[B:].T)


def timeline_oracle(table, state, asked, k, B, what, b0, bw, t0=I64_MIN, t1=I64_MAX, vals=None):
    """The four outputs of one window as the C entry lays them out for K = k: cnt / sum / max [k, B, 2], out
    [k, 2, 2]; asked: pod-op codes, -1 for the window's own traces.  state None: an empty window (zeros)."""
    cnt, tot, mx = (np.zeros((k, B, 2), np.int64) for _ in range(3))
    out = np.zeros((k, 2, 2), np.int64)
    if state is not None:
        state = np.asarray(state)
        ts, te = trace_times(table)
        tb = np.array([bucket_of(x, b0, bw, B) for x in ts.tolist()], np.int64)
        v = lc.values(table, what) if vals is None else vals
        st = np.where(lc.in_window(table, t0, t1), state[table.trace], 0)
        live = np.flatnonzero((state == 1) | (state == 2))
        with np.errstate(over="ignore"):
            tv = te - ts   # (int64: wraps)
        for j, p in enumerate(asked):
            if p < 0:
                cnt[j], tot[j], mx[j], out[j] = _hist(tb[live], state[live].astype(np.int64) - 1, tv[live], B)
            else:
                r = np.flatnonzero((table.podop == p) & (st > 0))
                cnt[j], tot[j], mx[j], out[j] = _hist(tb[table.trace[r]], st[r].astype(np.int64) - 1, v[r], B)
    return types.SimpleNamespace(cnt=cnt, sum=tot, max=mx, out=out)


FIELDS = ("cnt", "sum", "max", "out")


def same(got, exp):
    """Exact integer equality of every output of a window."""
    for f in FIELDS:
        a, b = getattr(got, f), getattr(exp, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tolist() == b.tolist(), f


def raw_bytes(out):
    return b"".join(getattr(o, f).tobytes() for o in out for f in FIELDS)


# ---------------------------------------------------------------------------------- case builders
def window(name):
    """kind_breakdown_cases.window: `ties`, `mid`, `ragged`, `one_trace` (window_exemplar_cases) or `fault`."""
    return kb.window(name)


def asked_ops(w):
    """kind_breakdown_cases.asked_ops: the top list, -1, the first top op again, an absent op."""
    return kb.asked_ops(w)


def grid(w, B, kind="default"):
    """(b0, bw) of a window's buckets: the Python layer's default -- origin t0, width (t1 - t0) // B + 1, every
    start of [t0, t1] in a bucket -- or an off-centre one that leaves rows before and after."""
    span = w.t1 - w.t0
    if kind == "default":
        return w.t0, span // B + 1
    return w.t0 + span // 3, span // (4 * B) + 1


@functools.lru_cache(maxsize=None)
def _values(name, what):
    v = lc.values(window(name).table, what)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def expected(name, B, what, kind="default"):
    w = window(name)
    b0, bw = grid(w, B, kind)
    return timeline_oracle(w.table, w.state, asked_ops(w), K_TOP, B, what, b0, bw, w.t0, w.t1, _values(name, what))


# the boundary table: its grid, its pod-op codes and its traces
B0, BW, NB = 10_000, 1_000, 4          # buckets [10_000, 11_000) ... [13_000, 14_000)
LON = 0                                # every trace's anchor row, which decides its side
EDGE = 1                               # two rows in each trace that starts on an edge of the bucket range
WRAP = 2                               # durations near +2^62 (abnormal) / -2^62 (normal): the sums wrap
NEG = 3                                # three negative durations in one bucket: max < 0
PAR = 4                                # the parent row of every run and of the WRAP rows: its self time is negative
IL1, IL2 = 5, 6                        # interleaved row by row
RUN = 7                                # RUN + i: a run of BOUNDARY_SIZES[i] consecutive rows of one key
NEVER = RUN + len(BOUNDARY_SIZES)      # a pod-op no row has
N_OPS = NEVER + 1
INTERLEAVED = 300
# trace code -> start; even codes below 12 and 14 are abnormal, odd ones and 15 normal
STARTS = {0: B0, 1: B0, 2: B0 - 1, 3: B0 - 1, 4: B0 + NB * BW - 1, 5: B0 + NB * BW - 1, 6: B0 + NB * BW, 7: B0 + NB * BW,
          8: B0 + 1500, 9: B0 + 1500, 10: B0 + 2500, 11: B0 + 2999, 12: B0 + 100, 13: 1_000_010, 14: B0 + 1000,
          15: B0 + 1999}
T_ABN, T_NOR, T_DROP, T_OUT = (0, 2, 4, 6, 8, 10, 14), (1, 3, 5, 7, 9, 11, 15), 12, 13
WIN = (0, 1_000_000)


@functools.lru_cache(maxsize=None)
def boundary():
    """A table of direct arrays built for the kernel's weak points (see the constants above).  Rows are in the
    order they are added: a run's rows are consecutive rows of one (op, bucket, side).  A trace ends 500 +
    its code ns after it starts.  One constant SLO of 1 ms per service-op: a trace of r rows is abnormal
    when its largest duration exceeds r * 1000; every trace's last row (its anchor, LON) decides that --
    r * 10_000 in an abnormal trace, 1 in a normal one, whose other durations stay <= 1000 (hugely negative
    ones included), 0 in the dropped trace, which has no positive duration."""
    from microrank_amd.spans import SpanTable
    import oracle as orc

    rng = np.random.default_rng(512)
    rows = []            # (trace, op, span, parent, duration)

    def row(t, op, parent=-1, dur=None):
        rows.append((t, op, len(rows), parent, int(rng.integers(1, 900)) if dur is None else int(dur)))
        return len(rows) - 1

    for t in range(8):                                               # the edges of the bucket range
        for j in range(2):
            row(t, EDGE, dur=(t + 1) * 10 + j)
    for j in range(3):
        row(T_DROP, EDGE, dur=-j)                                    # inside the window, state 0
    for j in range(2):
        row(T_OUT, EDGE, dur=50 + j)                                 # outside the window
    sizes = list(BOUNDARY_SIZES)
    for t, shift in ((8, 0), (9, 3)):                                # the runs
        for i in range(len(sizes)):
            p = row(t, PAR)
            for _ in range(sizes[(i + shift) % len(sizes)]):
                row(t, RUN + i, p)
    for t in (10, 11):                                               # two ops, row by row
        for _ in range(INTERLEAVED):
            row(t, IL1)
            row(t, IL2)
    p = row(14, PAR, dur=100)
    for k in range(3):
        row(14, WRAP, p, BIG + 7 * k)
    p = row(15, PAR, dur=100)
    for k in range(3):
        row(15, WRAP, p, -BIG - 5 * k)
    for d in (-5, -9, -2):
        row(15, NEG, dur=d)
    for t in range(16):                                              # the anchors
        r = sum(1 for x in rows if x[0] == t) + 1
        row(t, LON, -1, r * 10_000 if t in T_ABN else 0 if t == T_DROP else 1)
    a = np.asarray(rows, dtype=object)
    tr, op = np.asarray(a[:, 0], np.int32), np.asarray(a[:, 1], np.int32)
    start = np.array([STARTS[int(t)] for t in tr], np.int64)
    names = [f"pod_op{o:02d}" for o in range(N_OPS)]
    table = SpanTable(tr, op, op.copy(), np.asarray(a[:, 2], np.int64), np.asarray(a[:, 3], np.int64),
                      np.asarray(a[:, 4], np.int64), start, start + 500 + tr, [f"t{i:02d}" for i in range(16)], names,
                      list(names))
    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, WIN[0], WIN[1],
                     {i: 1.0 for i in range(N_OPS)})
    state = kb.state_of(16, res[1], res[2])
    return types.SimpleNamespace(name="boundary", table=table, a3=np.ones(N_OPS, np.float64), ok=np.ones(N_OPS, np.uint8),
                                 t0=WIN[0], t1=WIN[1], state=state)


def boundary_ops():
    """Every op with a rule of its own; EDGE and -1 twice."""
    return [EDGE, -1, WRAP, NEG, PAR, IL1, IL2] + [RUN + i for i in range(len(BOUNDARY_SIZES))] + [LON, NEVER, EDGE, -1]


# (b0, bw, B): the hand-checked grid; one-ns buckets; the widest buckets from the smallest origin, where every
# positive start has delta = start + 2^63 and falls in bucket 2 -- inside four buckets, after two
GRIDS = {"main": (B0, BW, NB), "ns": (B0, 1, 512), "wide4": (I64_MIN, BIG, 4), "wide2": (I64_MIN, BIG, 2)}


@functools.lru_cache(maxsize=None)
def boundary_expected(grid_name, what):
    b = boundary()
    b0, bw, B = GRIDS[grid_name]
    asked = boundary_ops()
    return timeline_oracle(b.table, b.state, asked, len(asked), B, what, b0, bw, b.t0, b.t1)


# ---------------------------------------------------------------------------------- GPU caller
def call(ctx, wins, ops, k, B, what, b0, bw, check=True, n_ops=None):
    """One raw mr_windows_timeline call over wins = [(DeviceSpans, t0, t1, a3, ok)] with the grids b0[i] / bw[i]:
    (status code, [outputs per window as timeline_oracle's namespace], status[n]).  The buffers start as
    garbage: the entry must write every word."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    n = len(wins)
    spans = (_lib.P * max(n, 1))(*[w[0].h for w in wins])
    t0 = np.array([w[1] for w in wins], np.int64)
    t1 = np.array([w[2] for w in wins], np.int64)
    a3 = (C.c_void_p * max(n, 1))(*[w[3].ctypes.data for w in wins])
    ok = (C.c_void_p * max(n, 1))(*[w[4].ctypes.data for w in wins])
    kk, bb = (k if 1 <= k <= 64 else 64), (B if 1 <= B <= 512 else 512)   # (the buffers of a call that must fail)
    cod = np.full((n, kk), 123456, np.int32)   # entries j >= n_ops[i] are ignored, whatever they hold
    n_ops = np.array([len(o) for o in ops] if n_ops is None else n_ops, np.int32)   # (n_ops: a count the lists cannot express)
    for i, o in enumerate(ops):
        cod[i, :min(len(o), kk)] = np.asarray(o, np.int32)[:kk]
    b0, bw = np.array(b0, np.int64).reshape(n), np.array(bw, np.int64).reshape(n)
    cnt, tot, mx = (np.full((n, kk, bb, 2), -7, np.int64) for _ in range(3))
    out = np.full((n, kk, 2, 2), -7, np.int64)
    status = np.full(n, -7, np.int32)
    code = what if isinstance(what, int) else lc.WHAT[what]
    rc = _lib.load().mr_windows_timeline(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                         ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, code, ptr(b0, C.c_int64),
                                         ptr(bw, C.c_int64), B, ptr(cnt, C.c_int64), ptr(tot, C.c_int64),
                                         ptr(mx, C.c_int64), ptr(out, C.c_int64), ptr(status, C.c_int32))
    if check:
        ctx.check(rc, "mr_windows_timeline")
    res = [types.SimpleNamespace(cnt=cnt[i], sum=tot[i], max=mx[i], out=out[i]) for i in range(n)]
    return rc, res, status
