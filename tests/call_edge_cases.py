"""Helpers of the call-evidence tests (mr_windows_call_edges, csrc/mr_call_edges.hip): the numpy oracle --
exactly the semantics of include/microrank_hip.h, from the span table's rows and a detector partition
(oracle.detect's lists as mr_detect's state[]) -- and the case builders.  Everything cached here is
shared between tests and read-only."""
import ctypes as C
import functools
import types

import numpy as np

import kind_breakdown_cases as kb
from kind_breakdown_cases import BOUNDARY_SIZES, K_TOP, MS, WINDOWS   # noqa: F401 -- the tests' shared figures

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
BIG = 1 << 62


# ---------------------------------------------------------------------------------- the oracle
def call_pairs(table, state, t0=I64_MIN, t1=I64_MAX):
    """(child rows, parent rows, side) of the window's call pairs: child c, parent r with parent[c] >= 0
    and span[r] == parent[c] (traceID ignored, every row of the spanID pairs), both rows in the window and
    both traces in state side + 1."""
    state = np.asarray(state)
    S = table.n_spans
    whole = t0 == I64_MIN and t1 == I64_MAX
    inw = np.ones(S, bool) if whole else (table.tstart >= t0) & (table.tend <= t1)
    sd = np.where(inw, state[table.trace], 0).astype(np.int64)
    order = np.argsort(table.span, kind="stable")
    srt = table.span[order]
    lo = np.searchsorted(srt, table.parent, "left")
    hi = np.searchsorted(srt, table.parent, "right")
    cnt = np.where(table.parent >= 0, hi - lo, 0)
    child = np.repeat(np.arange(S), cnt)
    local = np.arange(child.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    par = order[np.repeat(lo, cnt) + local]
    keep = (sd[child] == sd[par]) & (sd[child] > 0)
    return child[keep], par[keep], sd[child[keep]] - 1


def edge_counts(table, state, t0=I64_MIN, t1=I64_MAX):
    """{(parent op, child op): (calls[2], dsum[2], dmax[2])} over the window, side 0 normal, 1 abnormal;
    int64 sums that wrap; dmax 0 where calls is 0.  Only edges with a call appear."""
    child, par, side = call_pairs(table, state, t0, t1)
    out = {}
    if child.size == 0:
        return out
    key = np.stack([table.podop[par].astype(np.int64), table.podop[child].astype(np.int64)], 1)
    uk, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    slot = inv * 2 + side
    calls = np.bincount(slot, minlength=2 * len(uk)).astype(np.int64)
    dur = table.duration[child].astype(np.int64)
    dsum = np.zeros(2 * len(uk), np.int64)
    with np.errstate(over="ignore"):
        np.add.at(dsum, slot, dur)   # (int64: wraps)
    dmax = np.full(2 * len(uk), I64_MIN, np.int64)
    np.maximum.at(dmax, slot, dur)
    dmax[calls == 0] = 0
    for e, (a, b) in enumerate(uk.tolist()):
        out[(a, b)] = (calls[2 * e:2 * e + 2].copy(), dsum[2 * e:2 * e + 2].copy(), dmax[2 * e:2 * e + 2].copy())
    return out


def call_oracle(table, state, asked, k, m, t0=I64_MIN, t1=I64_MAX, edges=None):
    """The seven outputs of one window as the C entry lays them out for K = k: peer [k, 2, m], calls / dsum /
    dmax [k, 2, m, 2], n / peers [k, 2], tot [k, 2, 2].  state None: an empty window (the padding)."""
    peer = np.full((k, 2, m), -1, np.int32)
    calls, dsum, dmax = (np.zeros((k, 2, m, 2), np.int64) for _ in range(3))
    n, peers, tot = np.zeros((k, 2), np.int32), np.zeros((k, 2), np.int32), np.zeros((k, 2, 2), np.int64)
    if state is not None:
        ed = edges if edges is not None else edge_counts(table, state, t0, t1)
        for j, p in enumerate(asked):
            for d in (0, 1):   # callers: edges (q -> p), peer q; callees: edges (p -> c), peer c
                sel = [(key[d], v) for key, v in ed.items() if key[1 - d] == p]   # key = (parent op, child op)
                sel.sort(key=lambda e: (-int(e[1][0][1]), int(e[1][0][0]), e[0]))
                peers[j, d] = len(sel)
                n[j, d] = min(m, len(sel))
                tot[j, d] = [sum(int(e[1][0][0]) for e in sel), sum(int(e[1][0][1]) for e in sel)]
                for r, (q, v) in enumerate(sel[:m]):
                    peer[j, d, r] = q
                    calls[j, d, r], dsum[j, d, r], dmax[j, d, r] = v
    return types.SimpleNamespace(peer=peer, calls=calls, dsum=dsum, dmax=dmax, n=n, peers=peers, tot=tot)


FIELDS = ("peer", "calls", "dsum", "dmax", "n", "peers", "tot")


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
    """The asked slots of a window's case: kind_breakdown_cases.asked_ops without its -1 -- the top list,
    the first top op again, an op absent from the window (where the window has one)."""
    return [c for c in kb.asked_ops(w) if c >= 0]


@functools.lru_cache(maxsize=None)
def edges(name):
    w = window(name)
    return edge_counts(w.table, w.state, w.t0, w.t1)


@functools.lru_cache(maxsize=None)
def expected(name, m):
    w = window(name)
    return call_oracle(w.table, w.state, asked_ops(w), K_TOP, m, w.t0, w.t1, edges(name))


# the boundary table's pod-op codes
LONELY = 0                      # every trace's anchor row: a root nobody calls
PA, CH = 1, 11                  # PA + i -> CH + i: the run edges, i < len(BOUNDARY_SIZES)
U1, U2, U3, V = 21, 22, 23, 24  # three rows share one spanID (U1, U2 abnormal, U3 normal); V its children
W1, W2 = 25, 26                 # W2's only parent row (W1) lies in a trace of the other side
OP, OC = 27, 28                 # OC's only parent row (OP) lies outside the window
ORPH = 29                       # an orphan
SELF = 30                       # SELF -> SELF
HUB = 31                        # 40 callers Q + j and 40 callees CC + j
Q, CC, NPEER = 32, 72, 40
DP, DC = 112, 113               # DC's only parent row (DP) lies in a dropped trace (state 0 inside the window)
NEVER = 114                     # a pod-op no row has
N_OPS = 115
WRAP_UP, WRAP_DOWN = 2, 3       # run edges whose abnormal durations are near +2^62 / normal ones near -2^62
INTERLEAVE_CAP = 300
# traces: abnormal 0, 2, 4, 7; normal 1, 3, 5, 8; 6 outside the window; 9 dropped (no positive duration)
T_ABN, T_NOR, T_OUT, T_DROP = (0, 2, 4, 7), (1, 3, 5, 8), 6, 9


def hub_calls(j):
    """(abnormal, normal) calls of the hub's peer j, in each direction: ties in the abnormal calls, broken
    by the normal calls, then (j and j + 12 agree in both) by the code."""
    return 1 + j % 4, (j // 4) % 3


@functools.lru_cache(maxsize=None)
def boundary():
    """A table of direct arrays built for the kernel's weak points (see the constants above).  Rows are in
    the order they are added: a run's child rows are consecutive rows of one (edge, side), the interleaved
    section alternates the two sides row by row.  One constant SLO of 1 ms per service-op: a trace of r
    rows is abnormal when its largest duration exceeds r * 1000; every trace's last row (its anchor, a
    LONELY root) decides that -- r * 10_000 in an abnormal trace, 1 in a normal one, whose other durations
    stay <= 1000 (hugely negative ones included)."""
    from microrank_amd.spans import SpanTable

    rng = np.random.default_rng(77)
    rows = []            # (trace, op, span, parent, duration)
    nspan = [0]

    def span():
        nspan[0] += 1
        return nspan[0] - 1

    def row(t, op, parent=-1, dur=None, sp=None):
        sp = span() if sp is None else sp
        rows.append((t, op, sp, parent, int(rng.integers(1, 900)) if dur is None else int(dur)))
        return sp

    def edge_dur(i, abnormal, k):
        if i == WRAP_UP and abnormal:
            return BIG + 7 * k
        if i == WRAP_DOWN and not abnormal:
            return -BIG - 5 * k
        return None

    sizes = list(BOUNDARY_SIZES)
    ns = len(sizes)
    for t, abnormal, shift in ((0, True, 0), (1, False, 3)):          # the runs
        for i in range(ns):
            p = row(t, PA + i)
            for k in range(sizes[(i + shift) % ns]):
                row(t, CH + i, p, edge_dur(i, abnormal, k))
    for i in range(ns):                                              # the same edges, no run longer than 1
        pa, pn = row(2, PA + i), row(3, PA + i)
        for k in range(min(sizes[i], INTERLEAVE_CAP)):
            row(2, CH + i, pa, edge_dur(i, True, k))
            row(3, CH + i, pn, edge_dur(i, False, k))
    shared = span()                                                  # one spanID, three rows
    row(4, U1, sp=shared)
    row(4, U2, sp=shared)
    row(5, U3, sp=shared)
    row(4, V, shared, 400)        # two abnormal pairs, nothing on the normal side
    row(5, V, shared, 40)         # one normal pair (its abnormal partners are on the other side)
    w1 = row(5, W1)
    row(4, W2, w1)                # the parent's trace is normal, the child's abnormal: no pair
    op_ = row(T_OUT, OP)
    row(4, OC, op_)               # the parent lies outside the window: no pair
    dp = row(T_DROP, DP, dur=0)
    row(4, DC, dp)                # the parent's trace is dropped: no pair
    row(4, ORPH, -1)              # an orphan
    for t in (4, 5):              # SELF -> SELF -> SELF
        s0 = row(t, SELF)
        s1 = row(t, SELF, s0)
        row(t, SELF, s1, -3 if t == 5 else None)
    for t, side in ((7, 0), (8, 1)):                                 # the hub
        h = row(t, HUB)
        for j in range(NPEER):
            c = hub_calls(j)[side]
            if c:
                q = row(t, Q + j)
                for _ in range(c):
                    row(t, HUB, q)
                    row(t, CC + j, h)
    for t in range(10):                                              # the anchors
        r = sum(1 for x in rows if x[0] == t) + 1
        row(t, LONELY, -1, r * 10_000 if t in T_ABN else 0 if t == T_DROP else 1)
    a = np.asarray(rows, dtype=object)
    tr = np.asarray(a[:, 0], np.int32)
    op = np.asarray(a[:, 1], np.int32)
    t0, t1 = 1_000_000, 2_000_000
    start = np.where(tr == T_OUT, t1 + 10, t0 + 100 * (tr.astype(np.int64) + 1))
    names = [f"pod_op{o:03d}" for o in range(N_OPS)]
    table = SpanTable(tr, op, op.copy(), np.asarray(a[:, 2], np.int64), np.asarray(a[:, 3], np.int64),
                      np.asarray(a[:, 4], np.int64), start, start + 500, [f"t{i}" for i in range(10)], names, list(names))
    import oracle as orc

    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, t0, t1,
                     {i: 1.0 for i in range(N_OPS)})
    state = kb.state_of(10, res[1], res[2])
    return types.SimpleNamespace(name="boundary", table=table, a3=np.ones(N_OPS, np.float64), ok=np.ones(N_OPS, np.uint8),
                                 t0=t0, t1=t1, state=state)


def boundary_ops():
    """Every op with a rule of its own; HUB twice."""
    ns = len(BOUNDARY_SIZES)
    return ([PA + i for i in range(ns)] + [CH + i for i in range(ns)] +
            [U1, U2, U3, V, W1, W2, OP, OC, ORPH, SELF, HUB, Q + 5, CC + 17, DP, DC, LONELY, NEVER, HUB])


@functools.lru_cache(maxsize=None)
def boundary_expected(m=32):
    b = boundary()
    asked = boundary_ops()
    return call_oracle(b.table, b.state, asked, len(asked), m, b.t0, b.t1)


WIDE_OPS = 4100


@functools.lru_cache(maxsize=None)
def wide():
    """4100 pod-ops (past the layout order's 4096) on 2050 traces of three rows, trace-level times: trace t
    calls 2t -> 2t + 1 and 2t + 1 -> (2t + 2) % 4100, so every op has a caller and a callee in two
    different traces; even traces are abnormal (5 ms against 3 ms expected), odd ones normal."""
    from microrank_amd.spans import SpanTable
    import oracle as orc

    nt = WIDE_OPS // 2
    t = np.arange(nt, dtype=np.int64)
    tr = np.repeat(t, 3).astype(np.int32)
    op = np.stack([2 * t, 2 * t + 1, (2 * t + 2) % WIDE_OPS], 1).reshape(-1).astype(np.int32)
    S = tr.size
    parent = np.where(np.arange(S) % 3 > 0, np.arange(S) - 1, -1).astype(np.int64)
    dur = np.where(np.repeat(t, 3) % 2 == 0, 5000, 500).astype(np.int64) - np.arange(S) % 3
    ts = np.repeat(t + 1000, 3)
    names = [f"pod_op{o:04d}" for o in range(WIDE_OPS)]
    table = SpanTable(tr, op, op.copy(), np.arange(S, dtype=np.int64), parent, dur, ts, ts + 10,
                      [f"t{i:04d}" for i in range(nt)], names, list(names))
    t0, t1 = int(ts.min()), int(ts.max()) + 10
    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, t0, t1,
                     {i: 1.0 for i in range(WIDE_OPS)})
    state = kb.state_of(nt, res[1], res[2])
    return types.SimpleNamespace(name="wide", table=table, a3=np.ones(WIDE_OPS, np.float64), ok=np.ones(WIDE_OPS, np.uint8),
                                 t0=t0, t1=t1, state=state)


WIDE_ASKED = [0, 1, 2, 4095, 4096, 4097, 4098, 4099, 4099]


# ---------------------------------------------------------------------------------- GPU caller
def call(ctx, wins, ops, k, m, check=True, n_ops=None):
    """One raw mr_windows_call_edges call over wins = [(DeviceSpans, t0, t1, a3, ok)]: (status code, [outputs
    per window as call_oracle's namespace], status[n]).  The buffers start as garbage: the entry must
    write every word."""
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
    n_ops = np.array([len(o) for o in ops] if n_ops is None else n_ops, np.int32)   # (n_ops: a count the lists cannot express)
    for i, o in enumerate(ops):
        cod[i, :min(len(o), kk)] = np.asarray(o, np.int32)[:kk]
    peer = np.full((n, kk, 2, mm), -7, np.int32)
    calls, dsum, dmax = (np.full((n, kk, 2, mm, 2), -7, np.int64) for _ in range(3))
    cnt, peers = np.full((n, kk, 2), -7, np.int32), np.full((n, kk, 2), -7, np.int32)
    tot = np.full((n, kk, 2, 2), -7, np.int64)
    status = np.full(n, -7, np.int32)
    rc = _lib.load().mr_windows_call_edges(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                           ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m, ptr(peer, C.c_int32),
                                           ptr(calls, C.c_int64), ptr(dsum, C.c_int64), ptr(dmax, C.c_int64),
                                           ptr(cnt, C.c_int32), ptr(peers, C.c_int32), ptr(tot, C.c_int64),
                                           ptr(status, C.c_int32))
    if check:
        ctx.check(rc, "mr_windows_call_edges")
    out = [types.SimpleNamespace(peer=peer[i], calls=calls[i], dsum=dsum[i], dmax=dmax[i], n=cnt[i], peers=peers[i],
                                 tot=tot[i]) for i in range(n)]
    return rc, out, status
