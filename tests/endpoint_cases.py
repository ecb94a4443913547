"""Helpers of the endpoint-evidence tests (mr_spans_entry_ops, mr_windows_endpoints; csrc/mr_endpoints.hip): the numpy
oracle -- exactly the definitions of include/microrank_hip.h, from the span table's rows and a detector partition
(oracle.detect's lists as mr_detect's state[]) -- and the case builders.  Tables are built directly from arrays: one
service-op per pod-op, a constant SLO of 1 ms, so a trace of r rows is abnormal when its largest duration exceeds
r * 1000 and dropped when it has no positive duration.  Everything cached here is shared between tests and read-only."""
import ctypes as C
import functools
import types

import numpy as np

import detect_cases as dc

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIG = 1 << 62
NONE = -2                       # MR_EP_NONE
TILE = 1024                     # the count pass's tile: EP_T * EP_U entries (traces)
EV_H = 1024                     # keys of the block's counter table: direct-mapped up to here
MS = (1, 8, 32)
WHOLE = (I64_MIN, I64_MAX)


def wrap(v):
    """A Python int as the int64 it wraps to."""
    return (int(v) + (1 << 63)) % (1 << 64) - (1 << 63)


# ---------------------------------------------------------------------------------- the oracle
def root_rows(table):
    return np.flatnonzero(np.asarray(table.parent) < 0)


def entry_rows(table):
    """[n_traces] the entry row of every trace: among its root rows the largest duration (int64), ties to the
    smallest row position; -1 for a trace without a root row."""
    out = np.full(table.n_traces, -1, np.int64)
    r = root_rows(table)
    dur = np.ascontiguousarray(np.asarray(table.duration, np.int64)[r])
    longest_first = ~(dur.view(np.uint64) ^ np.uint64(1 << 63))   # (order-reversing on int64, -2^63 included)
    order = np.lexsort((r, longest_first, np.asarray(table.trace)[r]))
    tr = np.asarray(table.trace)[r][order]
    first = np.flatnonzero(np.r_[True, tr[1:] != tr[:-1]]) if tr.size else np.zeros(0, np.int64)
    out[tr[first]] = r[order][first]
    return out


def entry_ops(table):
    """[n_traces] int32: the endpoint of every trace, NONE without a root row."""
    rows = entry_rows(table)
    return np.where(rows >= 0, np.asarray(table.podop)[np.maximum(rows, 0)], NONE).astype(np.int32)


def entry_ops_loops(table):
    """entry_ops by plain Python loops over the rows."""
    best = {}
    for r in range(table.n_spans):
        if int(table.parent[r]) >= 0:
            continue
        t, d = int(table.trace[r]), int(table.duration[r])
        if t not in best or d > best[t][0]:
            best[t] = (d, r)
    return [int(table.podop[best[t][1]]) if t in best else NONE for t in range(table.n_traces)]


def trace_values(table):
    """[n_traces] Python ints: d(t) = tend - tstart at trace level as the int64 it wraps to (0 for a code without
    rows, which no window selects)."""
    d = [0] * table.n_traces
    for t, a, b in zip(np.asarray(table.trace).tolist(), np.asarray(table.tstart).tolist(), np.asarray(table.tend).tolist()):
        d[t] = wrap(b - a)
    return d


def traces_with(table, p):
    """The trace codes with at least one row of pod-op p."""
    return np.unique(np.asarray(table.trace)[np.asarray(table.podop) == p])


def slot_counts(table, state, p, ep=None, d=None):
    """{endpoint: [cnt[2], sum[2], max[2]]} of one asked slot (p = -1: every trace of the window), Python ints, sums
    not yet wrapped."""
    ep = entry_ops(table) if ep is None else ep
    d = trace_values(table) if d is None else d
    sel = np.flatnonzero(np.asarray(state) > 0) if p < 0 else traces_with(table, p)
    acc = {}
    for t in sel.tolist():
        st = int(state[t])
        if st == 0:
            continue
        a = acc.setdefault(int(ep[t]), [[0, 0], [0, 0], [None, None]])
        a[0][st - 1] += 1
        a[1][st - 1] += d[t]
        a[2][st - 1] = d[t] if a[2][st - 1] is None else max(a[2][st - 1], d[t])
    return acc


def order_key(e, a):
    """abnormal count descending, normal count ascending, code ascending with NONE last."""
    return (-a[0][1], a[0][0], e if e != NONE else 1 << 40)


def endpoint_oracle(table, state, asked, k, m):
    """The outputs of one window as the C entry lays them out for K = k: op [k, m], cnt / sum / max [k, m, 2],
    n / live [k], tot [k, 2, 3].  state None: an empty window (the padding)."""
    op = np.full((k, m), -1, np.int32)
    cnt, tot, mx = (np.zeros((k, m, 2), np.int64) for _ in range(3))
    n, live = np.zeros(k, np.int32), np.zeros(k, np.int32)
    total = np.zeros((k, 2, 3), np.int64)
    if state is not None:
        ep, d = entry_ops(table), trace_values(table)
        memo = {}
        for j, p in enumerate(asked):
            if p not in memo:
                memo[p] = slot_counts(table, state, p, ep, d)
            acc = memo[p]
            order = sorted(acc, key=lambda e: order_key(e, acc[e]))
            live[j], n[j] = len(order), min(m, len(order))
            for x, e in enumerate(order[:m]):
                a = acc[e]
                op[j, x] = e
                for side in (0, 1):
                    cnt[j, x, side], tot[j, x, side], mx[j, x, side] = a[0][side], wrap(a[1][side]), a[2][side] or 0
            for side in (0, 1):
                on = [acc[e][2][side] for e in order if acc[e][0][side] > 0]
                total[j, side] = [sum(acc[e][0][side] for e in order), wrap(sum(acc[e][1][side] for e in order)),
                                  max(on) if on else 0]
    return types.SimpleNamespace(op=op, cnt=cnt, sum=tot, max=mx, n=n, live=live, tot=total)


FIELDS = ("op", "cnt", "sum", "max", "n", "live", "tot")


def same(got, exp):
    """Exact integer equality of every output of a window."""
    for f in FIELDS:
        a, b = getattr(got, f), getattr(exp, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tolist() == b.tolist(), f


def raw_bytes(out):
    return b"".join(getattr(o, f).tobytes() for o in out for f in FIELDS)


def as_dict(e, j):
    """Entry j of an oracle answer as windows_endpoints' dict."""
    ent = [(None if int(e.op[j, r]) == NONE else int(e.op[j, r]), int(e.cnt[j, r, 1]), int(e.cnt[j, r, 0]),
            int(e.sum[j, r, 1]), int(e.sum[j, r, 0]), int(e.max[j, r, 1]), int(e.max[j, r, 0])) for r in range(int(e.n[j]))]
    v = e.tot[j]
    return {"entries": ent, "live": int(e.live[j]),
            "total": (int(v[1, 0]), int(v[0, 0]), int(v[1, 1]), int(v[0, 1]), int(v[1, 2]), int(v[0, 2]))}


def state_of(table, t0, t1, a3=None, ok=None):
    """oracle.detect's partition of [t0, t1] as mr_detect's state[] (None: the empty window), read-only."""
    a3, ok = slo(table) if a3 is None else (a3, ok)
    st = dc.detect_oracle(table, t0, t1, a3, ok)[0]
    if st is not None:
        st.setflags(write=False)
    return st


def slo(table):
    return np.ones(table.n_svcops, np.float64), np.ones(table.n_svcops, np.uint8)


# ---------------------------------------------------------------------------------- case builders
class Rows:
    """Rows of a table in the order they are added: add() returns the row's spanID (= its position)."""

    def __init__(self):
        self.rows, self.times = [], {}

    def add(self, t, op, dur, parent=-1):
        self.rows.append([t, op, len(self.rows), parent, int(dur)])
        return len(self.rows) - 1

    def trace(self, t, op, side, extra=(), ts=None, te=None):
        """A trace with one root of pod-op `op` that decides its side ('a' abnormal, 'n' normal, 'd' dropped) and
        children (pod-op, count) under it; returns the root's row."""
        rows = 1 + sum(c for _, c in extra)
        root = self.add(t, op, {"a": rows * 10_000, "n": 500, "d": 0}[side])
        for o, c in extra:
            for _ in range(c):
                self.add(t, o, 0 if side == "d" else 7, root)
        self.times[t] = (1000 + 10 * t if ts is None else ts, 1400 + 13 * t if te is None else te)
        return root

    def table(self, n_podops=None, order=None):
        a = np.asarray(self.rows, dtype=object)
        tr = np.asarray(a[:, 0], np.int32)
        ts = np.asarray([self.times[int(t)][0] for t in tr], dtype=object)
        te = np.asarray([self.times[int(t)][1] for t in tr], dtype=object)
        p = np.arange(len(self.rows)) if order is None else np.asarray(order)
        pod = np.asarray(a[:, 1], np.int32)
        npo = int(pod.max()) + 1 if n_podops is None else n_podops
        return dc.make_table(tr[p], pod[p], np.asarray(a[:, 4], np.int64)[p], ts[p].astype(np.int64), te[p].astype(np.int64),
                             podop=pod[p], span=np.asarray(a[:, 2], np.int64)[p], parent=np.asarray(a[:, 3], np.int64)[p],
                             n_podops=npo, n_svcops=npo)


def _case(name, table, t0=I64_MIN, t1=I64_MAX, **kw):
    a3, ok = slo(table)
    return types.SimpleNamespace(name=name, table=table, a3=a3, ok=ok, t0=t0, t1=t1, state=state_of(table, t0, t1, a3, ok), **kw)


# traces of index(): what each is there for, and its endpoint
IX_LATER, IX_TIE, IX_NEG, IX_BIG, IX_CYCLE, IX_ELSEWHERE, IX_CHILD_LONGER = range(7)
IX_EXPECT = [3, 4, 6, 8, NONE, NONE, 11]


@functools.lru_cache(maxsize=None)
def index():
    """One trace per rule of the entry row (IX_*; IX_EXPECT their endpoints by hand)."""
    r = Rows()
    r.add(IX_LATER, 2, 100)                      # two root rows, the longer one later
    r.add(IX_LATER, 3, 30_000)
    r.add(IX_TIE, 4, 25_000)                     # two root rows of equal duration: the smaller row wins
    r.add(IX_TIE, 5, 25_000)
    root = r.add(IX_NEG, 6, -5)                  # a negative root duration; its child is longer and no root
    r.add(IX_NEG, 7, 30_000, root)
    r.add(IX_BIG, 9, -BIG)                       # root durations at -2^62, +2^62, 2^62 - 1
    r.add(IX_BIG, 8, BIG)
    r.add(IX_BIG, 10, BIG - 1)
    a = r.add(IX_CYCLE, 1, 30_000, len(r.rows) + 1)   # a two-span parent cycle: no root row
    r.add(IX_CYCLE, 2, 5, a)
    r.add(IX_ELSEWHERE, 1, 30_000, 0)            # every parent resolves to another trace's span: no root row
    r.add(IX_ELSEWHERE, 2, 5, 2)
    root = r.add(IX_CHILD_LONGER, 11, 50)
    r.add(IX_CHILD_LONGER, 12, 40_000, root)
    for t in range(7):
        r.times[t] = (1000 + t, 2000 + 3 * t)
    return _case("index", r.table())


@functools.lru_cache(maxsize=None)
def one_row():
    r = Rows()
    r.trace(0, 0, "a")
    return _case("one_row", r.table())


def unknown_parent_frame():
    """A reference-schema frame: trace t1's only span names a ParentSpanId that is no spanID of the table (a root),
    trace t2's root is its first span."""
    import pandas as pd

    t = pd.Timestamp("2024-01-01")
    return pd.DataFrame({"traceID": ["t1", "t2", "t2"], "spanID": ["a", "b", "c"], "ParentSpanId": ["zz", None, "b"],
                         "serviceName": ["s", "s", "s"], "operationName": ["x", "y", "z"], "podName": ["p", "p", "p"],
                         "duration": [5000, 10, 20], "startTime": [t, t, t], "endTime": [t, t, t]})


@functools.lru_cache(maxsize=None)
def order_table(name):
    """detect_cases' interleaved table in one stored order (trace-level times): many root rows per trace, the
    300-row trace's more than a block of rows apart."""
    return _case("order_" + name, dc.order_table(name, True), *dc.order_windows(dc.order_table(name, True))[0])


def root_spread(table):
    """The largest distance in rows between two root rows of one trace."""
    r = root_rows(table)
    lo, hi = np.full(table.n_traces, I64_MAX), np.full(table.n_traces, -1)
    np.minimum.at(lo, table.trace[r], r)
    np.maximum.at(hi, table.trace[r], r)
    return int((hi - lo)[hi >= 0].max())


# distinct(): endpoint E_D; X has 1, 2 and 70 spans in traces 0..2 (abnormal, normal, abnormal); trace 3 has no X
E_D, X_D, Y_D = 0, 5, 6


@functools.lru_cache(maxsize=None)
def distinct():
    r = Rows()
    r.trace(0, E_D, "a", [(X_D, 1)])
    r.trace(1, E_D, "n", [(X_D, 2), (Y_D, 1)])
    r.trace(2, E_D, "a", [(X_D, 70)])
    r.trace(3, E_D, "n", [(Y_D, 3)])
    return _case("distinct", r.table())


# ranked(): endpoints 1, 2 tie at (2 abnormal, 1 normal) with the traces without a root row; 3 is live on the
# normal side only; 4 has (3, 0); X_R is on every trace; times grow with the trace code
X_R, GONE_R = 6, 7


@functools.lru_cache(maxsize=None)
def ranked():
    r = Rows()
    t = 0
    for e, sides in ((1, "aan"), (2, "aan"), (3, "nnn"), (4, "aaa")):
        for s in sides:
            r.trace(t, e, s, [(X_R, 2)])
            t += 1
    for s in "aan":                              # no root row: a two-span cycle (and X_R under it)
        a = r.add(t, 5, 40_000 if s == "a" else 300, len(r.rows) + 1)
        b = r.add(t, 5, 7, a)
        r.add(t, X_R, 7, b)
        r.times[t] = (1000 + 10 * t, 1400 + 13 * t)
        t += 1
    r.trace(t, 4, "d", [(X_R, 1)])               # dropped: no positive duration
    return _case("ranked", r.table(n_podops=GONE_R + 1), 0, 10_000)


def ranked_windows():
    """(the whole range, its first half -- traces left out --, an empty window, a second cut) of ranked()."""
    return [(0, 10_000), (0, 1400 + 13 * 7), (-50, -10), (1000 + 10 * 3, 10_000)]


N_WIDE = 600
X_W = N_WIDE


@functools.lru_cache(maxsize=None)
def wide():
    """600 endpoints (pod-ops 0..599) of 1..3 traces each, X_W and one of 64 further ops on every trace: one slot
    holds 601 * 2 keys, past the block's direct-mapped table."""
    rng = np.random.default_rng(77)
    r = Rows()
    t = 0
    for e in range(N_WIDE):
        for _ in range(int(rng.integers(1, 4))):
            r.trace(t, e, "an"[int(rng.integers(0, 2))], [(X_W, int(rng.integers(1, 3))), (X_W + 1 + t % 64, 1)])
            t += 1
    return _case("wide", r.table(n_podops=X_W + 66), 0, 1 << 40)


def wide_asked():
    """64 asked codes: duplicates among them, -1 in the middle."""
    ops = [X_W, 3, X_W + 1, X_W + 2, 3, X_W] + list(range(X_W + 3, X_W + 29))
    ops = ops + [-1] + list(range(X_W + 29, X_W + 59)) + [-1]
    assert len(ops) == 64
    return ops


@functools.lru_cache(maxsize=None)
def cut(n):
    """n traces of one row each: n entries of the distinct pod-op lists too.  Endpoint t % 7, sides by t % 3."""
    r = Rows()
    for t in range(n):
        r.trace(t, t % 7, "and"[t % 3], ts=t, te=2 * t + 5)
    return _case(f"cut{n}", r.table(), 0, 1 << 40)


@functools.lru_cache(maxsize=None)
def wrapping():
    """Two abnormal traces and a normal one with tstart = -2^62, tend = 2^62: d wraps to -2^63, the sums wrap again."""
    r = Rows()
    for t, s in enumerate("aan"):
        r.trace(t, 1, s, [(2, 1)], ts=-BIG, te=BIG)
    r.trace(3, 1, "a", [(2, 1)], ts=5, te=9)
    return _case("wrapping", r.table())


# ---------------------------------------------------------------------------------- GPU callers
def call(ctx, wins, ops, k, m, check=True, n_ops=None):
    """One raw mr_windows_endpoints call over wins = [(DeviceSpans, t0, t1, a3, ok)]: (status code, [outputs per
    window as endpoint_oracle's namespace], status[n]).  The buffers start as garbage: the entry must write every
    word."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    n = len(wins)
    spans = (_lib.P * max(n, 1))(*[w[0].h for w in wins])
    t0 = np.array([w[1] for w in wins], np.int64)
    t1 = np.array([w[2] for w in wins], np.int64)
    a3 = (C.c_void_p * max(n, 1))(*[w[3].ctypes.data for w in wins])
    ok = (C.c_void_p * max(n, 1))(*[w[4].ctypes.data for w in wins])
    kk, mm = (k if 1 <= k <= 64 else 64), (m if 1 <= m <= 32 else 32)   # (the buffers of a call that must fail)
    cod = np.full((n, kk), 123456, np.int32)   # entries j >= n_ops[i] are ignored, whatever they hold
    n_ops = np.array([len(o) for o in ops] if n_ops is None else n_ops, np.int32)
    for i, o in enumerate(ops):
        cod[i, :min(len(o), kk)] = np.asarray(o, np.int32)[:kk]
    eop = np.full((n, kk, mm), -7, np.int32)
    cnt, tot, mx = (np.full((n, kk, mm, 2), -7, np.int64) for _ in range(3))
    cn, live = np.full((n, kk), -7, np.int32), np.full((n, kk), -7, np.int32)
    total = np.full((n, kk, 2, 3), -7, np.int64)
    status = np.full(n, -7, np.int32)
    rc = _lib.load().mr_windows_endpoints(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                          ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m, ptr(eop, C.c_int32),
                                          ptr(cnt, C.c_int64), ptr(tot, C.c_int64), ptr(mx, C.c_int64), ptr(cn, C.c_int32),
                                          ptr(live, C.c_int32), ptr(total, C.c_int64), ptr(status, C.c_int32))
    if check:
        ctx.check(rc, "mr_windows_endpoints")
    res = [types.SimpleNamespace(op=eop[i], cnt=cnt[i], sum=tot[i], max=mx[i], n=cn[i], live=live[i], tot=total[i])
           for i in range(n)]
    return rc, res, status


def win_of(dev, w, t0=None, t1=None):
    return (dev, w.t0 if t0 is None else t0, w.t1 if t1 is None else t1, w.a3, w.ok)
