"""Helpers of the timeline-quantile tests (mr_windows_timeline_q, csrc/mr_timeline.hip): the numpy oracle --
np.quantile of the int64 values of every (asked entry, bucket, side), built from timeline_cases' bucket rule and
trace times and latency_cases' values and window test -- and the raw caller.  Everything cached here is shared
between tests and read-only."""
import ctypes as C
import functools
import types

import numpy as np

import latency_cases as lc
import timeline_cases as tc
from timeline_cases import K_TOP, NAMES   # noqa: F401 -- the tests' shared figures

QS = lc.QS
METHODS = ("linear", "lower", "higher")
# (B, what, method) of the named-window cases: B in (1, 7, 30) with both values and the three methods, and one
# case of 512 buckets
CASES = [(B, what, m) for B in (1, 7, 30) for what in tc.WHATS for m in METHODS] + [(512, "self", "linear")]


# ---------------------------------------------------------------------------------- the oracle
def _groups(bk, side, val, B):
    """{(bucket, side): the int64 values} of the selected triples with a bucket inside the range."""
    keep = bk < B
    g = bk[keep] * 2 + side[keep]
    v = val[keep]
    order = np.argsort(g, kind="stable")
    g, v = g[order], v[order]
    cut = np.flatnonzero(np.diff(g)) + 1
    return {(int(x[0]) >> 1, int(x[0]) & 1): y for x, y in zip(np.split(g, cut), np.split(v, cut)) if x.size}


def quantile_oracle(table, state, asked, k, B, what, b0, bw, qs, method, t0=tc.I64_MIN, t1=tc.I64_MAX, vals=None):
    """tl_q of one window as the C entry lays it out for K = k, and the counts it implies: (q [k, B, 2, n_q]
    float64, cnt [k, B, 2] int64); asked: pod-op codes, -1 for the window's own traces.  state None: an empty
    window (zeros).  A class without a value answers 0.0."""
    qs = np.asarray(qs, np.float64).reshape(-1)
    out = np.zeros((k, B, 2, qs.size), np.float64)
    cnt = np.zeros((k, B, 2), np.int64)
    if state is None:
        return out, cnt
    state = np.asarray(state)
    ts, te = tc.trace_times(table)
    tb = np.array([tc.bucket_of(x, b0, bw, B) for x in ts.tolist()], np.int64)
    v = lc.values(table, what) if vals is None else vals
    st = np.where(lc.in_window(table, t0, t1), state[table.trace], 0)
    live = np.flatnonzero((state == 1) | (state == 2))
    with np.errstate(over="ignore"):
        tv = te - ts   # (int64: wraps)
    for j, p in enumerate(asked):
        if p < 0:
            groups = _groups(tb[live], state[live].astype(np.int64) - 1, tv[live], B)
        else:
            r = np.flatnonzero((table.podop == p) & (st > 0))
            groups = _groups(tb[table.trace[r]], st[r].astype(np.int64) - 1, v[r].astype(np.int64), B)
        for (b, side), a in groups.items():
            cnt[j, b, side] = a.size
            out[j, b, side] = np.quantile(a, qs, method=method)
    return out, cnt


@functools.lru_cache(maxsize=None)
def expected(name, B, what, method, kind="default"):
    """(q, cnt) of a named window over its asked ops, K_TOP slots, lc.QS."""
    w = tc.window(name)
    b0, bw = tc.grid(w, B, kind)
    q, cnt = quantile_oracle(w.table, w.state, tc.asked_ops(w), K_TOP, B, what, b0, bw, QS, method, w.t0, w.t1,
                             tc._values(name, what))
    q.setflags(write=False)
    cnt.setflags(write=False)
    return q, cnt


def boundary_asked(what="duration"):
    """timeline_cases.boundary_ops() minus WRAP, whose durations span 2^63: no key holds them beside a class.
    For self time also minus PAR, WRAP's parent: its self time is 100 minus the children's, just as wide."""
    gone = (tc.WRAP,) if what == "duration" else (tc.WRAP, tc.PAR)
    return [c for c in tc.boundary_ops() if c not in gone]


def boundary_kept(what="duration"):
    """The places of boundary_asked(what) in timeline_cases.boundary_ops()."""
    asked = boundary_asked(what)
    return [j for j, c in enumerate(tc.boundary_ops()) if c in asked]


@functools.lru_cache(maxsize=None)
def boundary_expected(grid_name, what, method):
    b = tc.boundary()
    b0, bw, B = tc.GRIDS[grid_name]
    asked = boundary_asked(what)
    q, cnt = quantile_oracle(b.table, b.state, asked, len(asked), B, what, b0, bw, QS, method, b.t0, b.t1)
    q.setflags(write=False)
    cnt.setflags(write=False)
    return q, cnt


def class_sizes(cnt):
    """Which of the sizes 0, 1, 2 and >= 100 the classes of a count array show."""
    c = np.asarray(cnt).reshape(-1)
    return {0: bool((c == 0).any()), 1: bool((c == 1).any()), 2: bool((c == 2).any()), 100: bool((c >= 100).any())}


# ---------------------------------------------------------------------------------- GPU caller
FIELDS = tc.FIELDS + ("q",)


def call(ctx, wins, ops, k, B, what, b0, bw, qs=QS, method="linear", check=True, n_ops=None, n_q=None):
    """One raw mr_windows_timeline_q call over wins = [(DeviceSpans, t0, t1, a3, ok)] with the grids b0[i] / bw[i]:
    (status code, [outputs per window: timeline_cases.call's namespace with q [k, B, 2, n_q]], status[n]).  Every
    output buffer starts as garbage: the entry must write every word."""
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
    n_ops = np.array([len(o) for o in ops] if n_ops is None else n_ops, np.int32)
    for i, o in enumerate(ops):
        cod[i, :min(len(o), kk)] = np.asarray(o, np.int32)[:kk]
    b0, bw = np.array(b0, np.int64).reshape(n), np.array(bw, np.int64).reshape(n)
    qv = np.ascontiguousarray(np.asarray(qs, np.float64).reshape(-1))
    nq = qv.size if n_q is None else n_q
    qq = nq if 1 <= nq <= 16 else 16
    cnt, tot, mx = (np.full((n, kk, bb, 2), -7, np.int64) for _ in range(3))
    out = np.full((n, kk, 2, 2), -7, np.int64)
    tq = np.full((n, kk, bb, 2, qq), -7.5, np.float64)
    status = np.full(n, -7, np.int32)
    wcode = what if isinstance(what, int) else lc.WHAT[what]
    mcode = method if isinstance(method, int) else lc.METHODS[method]
    rc = _lib.load().mr_windows_timeline_q(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                           ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, wcode, ptr(b0, C.c_int64),
                                           ptr(bw, C.c_int64), B, ptr(qv, C.c_double), nq, mcode, ptr(cnt, C.c_int64),
                                           ptr(tot, C.c_int64), ptr(mx, C.c_int64), ptr(out, C.c_int64),
                                           ptr(tq, C.c_double), ptr(status, C.c_int32))
    if check:
        ctx.check(rc, "mr_windows_timeline_q")
    res = [types.SimpleNamespace(cnt=cnt[i], sum=tot[i], max=mx[i], out=out[i], q=tq[i]) for i in range(n)]
    return rc, res, status


def raw_bytes(out):
    """The bytes of all five outputs of a call's windows."""
    return b"".join(getattr(o, f).tobytes() for o in out for f in FIELDS)
