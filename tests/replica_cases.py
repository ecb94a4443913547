"""Helpers of the replica-evidence tests (mr_windows_replicas, csrc/mr_replicas.hip): the numpy oracle --
exactly the semantics of include/microrank_hip.h, from the span table's rows and a detector partition
(oracle.detect's lists as mr_detect's state[]) -- and the case builders.  Everything cached here is shared
between tests and read-only."""
import ctypes as C
import functools
import types

import numpy as np

import kind_breakdown_cases as kb
import latency_cases as lc
from kind_breakdown_cases import BOUNDARY_SIZES, K_TOP, MS   # noqa: F401 -- the tests' shared figures

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIG = 1 << 62
WHATS = ("duration", "self")


def wrap(v):
    """A Python int as the int64 it wraps to."""
    return (int(v) + (1 << 63)) % (1 << 64) - (1 << 63)


# ---------------------------------------------------------------------------------- the oracle
def sv_map(table):
    """(sv[n_podops], ambiguous pod-op codes): sv(p) the service-op code on ALL the table's rows whose pod-op
    is p, -1 for a pod-op without a row; a pod-op whose rows carry two service-op codes is ambiguous."""
    lo = np.full(table.n_podops, np.iinfo(np.int32).max, np.int64)
    hi = np.full(table.n_podops, -1, np.int64)
    np.minimum.at(lo, table.podop, table.svcop)
    np.maximum.at(hi, table.podop, table.svcop)
    return np.where(hi >= 0, lo, -1), np.flatnonzero((hi >= 0) & (lo != hi))


def replicas_of(sv, s):
    """R(s) in code order."""
    return np.flatnonzero(sv == s) if s >= 0 else np.zeros(0, np.int64)


def podop_counts(table, state, what, t0=I64_MIN, t1=I64_MAX, vals=None):
    """cnt / sum / max [n_podops, 2] of the selected rows of every (pod-op, side): int64 sums that wrap, max 0
    where cnt is 0."""
    v = lc.values(table, what) if vals is None else vals
    st = np.where(lc.in_window(table, t0, t1), np.asarray(state)[table.trace], 0)
    r = np.flatnonzero(st > 0)
    side = st[r].astype(np.int64) - 1
    n = table.n_podops
    cnt, tot = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
    mx = np.full((n, 2), I64_MIN, np.int64)
    np.add.at(cnt, (table.podop[r], side), 1)
    with np.errstate(over="ignore"):
        np.add.at(tot, (table.podop[r], side), v[r])   # (int64: wraps)
    np.maximum.at(mx, (table.podop[r], side), v[r])
    mx[cnt == 0] = 0
    return cnt, tot, mx


def ordered_live(cnt, reps):
    """The live replicas of reps under the order: abnormal count descending, normal ascending, code ascending."""
    live = [int(q) for q in reps if cnt[q, 0] + cnt[q, 1] > 0]
    return sorted(live, key=lambda q: (-int(cnt[q, 1]), int(cnt[q, 0]), q))


def replica_oracle(table, state, asked, k, m, what, t0=I64_MIN, t1=I64_MAX, vals=None):
    """The outputs of one window as the C entry lays them out for K = k: pod [k, m], cnt / sum / max [k, m, 2],
    n / live / all / place [k], own / tot [k, 2, 3].  state None: an empty window (the padding)."""
    pod = np.full((k, m), -1, np.int32)
    cnt, tot, mx = (np.zeros((k, m, 2), np.int64) for _ in range(3))
    n, live, every = (np.zeros(k, np.int32) for _ in range(3))
    place = np.full(k, -1, np.int32)
    own, total = np.zeros((k, 2, 3), np.int64), np.zeros((k, 2, 3), np.int64)
    if state is not None:
        sv, bad = sv_map(table)
        assert bad.size == 0
        c, s, x = podop_counts(table, state, what, t0, t1, vals)
        for j, p in enumerate(asked):
            reps = replicas_of(sv, sv[p])
            if reps.size == 0:
                continue
            order = ordered_live(c, reps)
            every[j], live[j], n[j] = reps.size, len(order), min(m, len(order))
            for e, q in enumerate(order[:m]):
                pod[j, e], cnt[j, e], tot[j, e], mx[j, e] = q, c[q], s[q], x[q]
            if p in order:
                place[j] = order.index(p)
            for side in (0, 1):
                own[j, side] = [c[p, side], s[p, side], x[p, side]]
                on = [q for q in order if c[q, side] > 0]
                total[j, side] = [sum(int(c[q, side]) for q in order), wrap(sum(int(s[q, side]) for q in order)),
                                  max(int(x[q, side]) for q in on) if on else 0]
    return types.SimpleNamespace(pod=pod, cnt=cnt, sum=tot, max=mx, n=n, live=live, all=every, place=place, own=own,
                                 tot=total)


FIELDS = ("pod", "cnt", "sum", "max", "n", "live", "all", "place", "own", "tot")


def same(got, exp):
    """Exact integer equality of every output of a window."""
    for f in FIELDS:
        a, b = getattr(got, f), getattr(exp, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tolist() == b.tolist(), f


def raw_bytes(out):
    return b"".join(getattr(o, f).tobytes() for o in out for f in FIELDS)


def as_dict(e, j):
    """Entry j of an oracle answer as windows_replicas' dict."""
    ent = [(int(e.pod[j, r]), int(e.cnt[j, r, 1]), int(e.cnt[j, r, 0]), int(e.sum[j, r, 1]), int(e.sum[j, r, 0]),
            int(e.max[j, r, 1]), int(e.max[j, r, 0])) for r in range(int(e.n[j]))]

    def six(v):
        return (int(v[1, 0]), int(v[0, 0]), int(v[1, 1]), int(v[0, 1]), int(v[1, 2]), int(v[0, 2]))

    return {"entries": ent, "live": int(e.live[j]), "all": int(e.all[j]), "place": int(e.place[j]), "own": six(e.own[j]),
            "total": six(e.tot[j])}


# ---------------------------------------------------------------------------------- case builders
def _case(name, table, a3, ok, state, t0, t1, **kw):
    state = np.array(state)
    state.setflags(write=False)
    return types.SimpleNamespace(name=name, table=table, a3=a3, ok=ok, t0=t0, t1=t1, state=state, **kw)


def abnormal_rows(table, state):
    return np.bincount(table.podop[np.asarray(state)[table.trace] == 2], minlength=table.n_podops)


def top_by_abnormal_rows(table, state, n=K_TOP):
    """The n pod-ops with the most abnormal rows (ties: the smaller code)."""
    rows = abnormal_rows(table, state)
    order = np.lexsort((np.arange(rows.size), -rows))
    return [int(c) for c in order[:n] if rows[c] > 0]


@functools.lru_cache(maxsize=None)
def pods3():
    """synth.window_pair(40, 2000, 3, pods=3): 36513 rows, 120 pod-ops, 40 service-ops of 3 replicas each."""
    from microrank_amd import synth

    topo, normal, abnormal = synth.window_pair(40, 2000, 3, pods=3)
    a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
    return _case("pods3", abnormal, a3, ok, state, t0, t1, topo=topo)


@functools.lru_cache(maxsize=None)
def wide(half=False):
    """synth.window_pair(12, 300, 7, pods=70): 2215 rows, 743 pod-ops with rows, 49..69 replicas per service-op.
    half: the window over the first half of its time range (live < all)."""
    from microrank_amd import synth

    _, normal, abnormal = synth.window_pair(12, 300, 7, pods=70)
    if not half:
        a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
        return _case("wide", abnormal, a3, ok, state, t0, t1)
    w = wide()
    t1 = w.t0 + (w.t1 - w.t0) // 2
    a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal, w.t0, t1)
    return _case("wide_half", w.table, a3, ok, state, t0, t1)


def wide_ops(w):
    """One pod-op of each service-op: the replica with the most abnormal rows (ties: the smaller code)."""
    sv, _ = sv_map(w.table)
    rows = abnormal_rows(w.table, w.state)
    ops = []
    for s in range(w.table.n_svcops):
        reps = replicas_of(sv, s)
        if reps.size:
            ops.append(int(reps[np.lexsort((reps, -rows[reps]))[0]]))
    return ops


@functools.lru_cache(maxsize=None)
def one_pod():
    """pods3 with the fault op's rows on abnormal traces relabelled to its pod 0 -- podop only, so the detector's
    state is what it was: one pod takes every abnormal row of the operation.  .pods: the op's three pod-op codes."""
    import dataclasses

    from microrank_amd import synth

    w = pods3()
    t = w.table
    fault = synth.fault_op_of(w.topo)
    mine = t.meta["op"] == fault
    pods = [int(np.unique(t.podop[mine & (t.meta["pod_k"] == k)])[0]) for k in range(3)]
    podop = t.podop.copy()
    podop[mine & (w.state[t.trace] == 2)] = pods[0]
    return _case("one_pod", dataclasses.replace(t, podop=podop), w.a3, w.ok, w.state, w.t0, w.t1, pods=pods)


@functools.lru_cache(maxsize=None)
def ambiguous():
    """pods3 with one row's svcop changed: its pod-op (.pod) has rows of two service-ops (.svcs)."""
    import dataclasses

    w = pods3()
    svcop = w.table.svcop.copy()
    row = 1234
    old = int(svcop[row])
    svcop[row] = (old + 1) % w.table.n_svcops
    pod = int(w.table.podop[row])
    return _case("ambiguous", dataclasses.replace(w.table, svcop=svcop), w.a3, w.ok, w.state, w.t0, w.t1, pod=pod,
                 svcs=sorted((old, int(svcop[row]))))


@functools.lru_cache(maxsize=None)
def span_times():
    """window_pair(40, 600, 3, pods=2, span_times=True): times vary within a trace (the row-level detector)."""
    from microrank_amd import synth

    _, normal, abnormal = synth.window_pair(40, 600, 3, pods=2, span_times=True)
    a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
    return _case("span_times", abnormal, a3, ok, state, t0, t1)


# the boundary table: service-op s holds the pod-ops whose svcop is s
S_LON = 0                               # pod-op LON: every trace's anchor row, which decides its side
S_IL = 1                                # IL1, IL2: two replicas interleaved row by row
S_WRAP = 2                              # WR_UP (durations near +2^62), WR_DOWN (near -2^62, its maximum negative), WR_PAR
S_DROP = 3                              # DR_LIVE, and DR_DEAD with rows only on dropped and outside traces: not live
S_RUN = 4                               # S_RUN + i: the replicas RUN_A + 2i, RUN_A + 2i + 1 with runs of BOUNDARY_SIZES[i] rows
LON, IL1, IL2, WR_UP, WR_DOWN, WR_PAR, DR_LIVE, DR_DEAD = range(8)
RUN_A = 8
NEVER = RUN_A + 2 * len(BOUNDARY_SIZES)   # a pod-op code without rows: table.take of a subset keeps the dictionaries
N_PODS = NEVER + 1
N_SVCS = S_RUN + len(BOUNDARY_SIZES) + 1  # (the last service-op: NEVER's, which no row has either)
INTERLEAVED = 300
# traces: abnormal 0, 2; normal 1, 3; 4 dropped (no positive duration); 5 outside the window
T_ABN, T_NOR, T_DROP, T_OUT = (0, 2), (1, 3), 4, 5
WIN = (0, 1_000_000)


@functools.lru_cache(maxsize=None)
def boundary():
    """A table of direct arrays built for the kernel's weak points (see the constants above).  Rows are in the
    order they are added: a run's rows are consecutive rows of one (replica, side).  One constant SLO of 1 ms per
    service-op: a trace of r rows is abnormal when its largest duration exceeds r * 1000; every trace's last row
    (its anchor, LON) decides that -- r * 10_000 in an abnormal trace, 1 in a normal one, whose other durations
    stay <= 1000, 0 in the dropped trace, which has no positive duration.  The table is a `take` of a larger one
    whose last row alone carries NEVER."""
    from microrank_amd.spans import SpanTable
    import oracle as orc

    rng = np.random.default_rng(640)
    rows = []            # (trace, pod-op, service-op, span, parent, duration)

    def row(t, op, sv, parent=-1, dur=None):
        rows.append((t, op, sv, len(rows), parent, int(rng.integers(1, 900)) if dur is None else int(dur)))
        return len(rows) - 1

    sizes = list(BOUNDARY_SIZES)
    for t, shift in ((0, 0), (1, 3)):                                # the runs: replica A in one key, then replica B
        for i in range(len(sizes)):
            p = row(t, WR_PAR, S_WRAP)
            for rep in (0, 1):
                for _ in range(sizes[(i + shift + rep) % len(sizes)]):
                    row(t, RUN_A + 2 * i + rep, S_RUN + i, p)
    for t in (2, 3):                                                 # two replicas, row by row
        for _ in range(INTERLEAVED):
            row(t, IL1, S_IL)
            row(t, IL2, S_IL)
    p = row(2, WR_PAR, S_WRAP, dur=100)
    for k in range(3):
        row(2, WR_UP, S_WRAP, p, BIG + 7 * k)                        # abnormal: the sum wraps
    p = row(3, WR_PAR, S_WRAP, dur=100)
    for k in range(3):
        row(3, WR_DOWN, S_WRAP, p, -BIG - 5 * k)                     # normal: the sum wraps, the maximum is negative
    for t in (0, 1):
        row(t, DR_LIVE, S_DROP)
    for _ in range(5):
        row(T_DROP, DR_DEAD, S_DROP, dur=-3)                         # inside the window, state 0
    for _ in range(2):
        row(T_OUT, DR_DEAD, S_DROP, dur=50)                          # outside the window
    for t in range(6):                                               # the anchors
        r = sum(1 for x in rows if x[0] == t) + 1
        row(t, LON, S_LON, -1, r * 10_000 if t in T_ABN else 0 if t == T_DROP else 1)
    row(5, NEVER, N_SVCS - 1, dur=1)                                 # (dropped by the take below)
    a = np.asarray(rows, dtype=object)
    tr = np.asarray(a[:, 0], np.int32)
    start = np.where(tr == T_OUT, 2_000_000, 1000 + tr).astype(np.int64)
    full = SpanTable(tr, np.asarray(a[:, 1], np.int32), np.asarray(a[:, 2], np.int32), np.asarray(a[:, 3], np.int64),
                     np.asarray(a[:, 4], np.int64), np.asarray(a[:, 5], np.int64), start, start + 500,
                     [f"t{i:02d}" for i in range(6)], [f"pod_op{o:02d}" for o in range(N_PODS)],
                     [f"svc_op{o:02d}" for o in range(N_SVCS)])
    table = full.take(np.arange(len(rows) - 1))
    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, WIN[0], WIN[1],
                     {i: 1.0 for i in range(N_SVCS)})
    state = kb.state_of(6, res[1], res[2])
    return _case("boundary", table, np.ones(N_SVCS, np.float64), np.ones(N_SVCS, np.uint8), state, WIN[0], WIN[1])


def boundary_ops():
    """Every replica with a rule of its own; IL1 twice; both replicas of a run; the code without rows."""
    return ([IL1, IL2, WR_UP, WR_DOWN, WR_PAR, DR_LIVE, DR_DEAD, LON] + [RUN_A + 2 * i for i in range(len(BOUNDARY_SIZES))] +
            [RUN_A + 1, NEVER, IL1])


CASES = {"pods3": pods3, "wide": wide, "one_pod": one_pod, "boundary": boundary}


def asked(name):
    """The asked list of a named case: its top list (the pod-ops with the most abnormal rows; for `wide` one
    pod-op per service-op; for `boundary` boundary_ops), the first op again, a replica of an already asked op,
    an op with no row in the window (where there is one) and a code without rows in the table (where there is
    one); `one_pod` asks the fault op's pod 1 too."""
    w = CASES[name]()
    if name == "boundary":
        return boundary_ops()
    sv, _ = sv_map(w.table)
    ops = wide_ops(w) if name == "wide" else top_by_abnormal_rows(w.table, w.state)
    sib = [int(q) for p in ops for q in replicas_of(sv, sv[p]) if q not in ops]
    ops = ops + [ops[0]] + sib[:1]
    gone = kb.absent_op(w.table, w.state)
    if gone is not None:
        ops.append(gone)
    if name == "one_pod":
        ops.append(w.pods[1])   # the fault op's pod 1: no abnormal row is left on it, its place is last
    return ops


@functools.lru_cache(maxsize=None)
def _values(name, what):
    v = lc.values(CASES[name]().table, what)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def expected(name, m, what, k=None):
    w = CASES[name]()
    ops = asked(name)
    return replica_oracle(w.table, w.state, ops, k or max(len(ops), 1), m, what, w.t0, w.t1, _values(name, what))


def brute_force(table, state, p, what, t0, t1):
    """The answer for one asked code by plain Python loops over the rows: (ordered live [(q, cnt[2], sum[2],
    max[2])], |R|)."""
    sv = {}
    for q, s in zip(table.podop.tolist(), table.svcop.tolist()):
        assert sv.setdefault(q, s) == s
    if p not in sv:
        return [], 0
    reps = sorted(q for q in sv if sv[q] == sv[p])
    v = lc.values(table, what).tolist()
    whole = t0 == I64_MIN and t1 == I64_MAX
    acc = {q: [[0, 0], [0, 0], [None, None]] for q in reps}
    for r in range(table.n_spans):
        q = int(table.podop[r])
        st = int(state[table.trace[r]])
        if q not in acc or st == 0 or not (whole or (table.tstart[r] >= t0 and table.tend[r] <= t1)):
            continue
        a = acc[q]
        a[0][st - 1] += 1
        a[1][st - 1] = wrap(a[1][st - 1] + v[r])
        a[2][st - 1] = v[r] if a[2][st - 1] is None else max(a[2][st - 1], v[r])
    live = [(q, a[0], a[1], [x or 0 for x in a[2]]) for q, a in acc.items() if sum(a[0]) > 0]
    live.sort(key=lambda e: (-e[1][1], e[1][0], e[0]))
    return live, len(reps)


# ---------------------------------------------------------------------------------- GPU caller
def call(ctx, wins, ops, k, m, what, check=True, n_ops=None):
    """One raw mr_windows_replicas call over wins = [(DeviceSpans, t0, t1, a3, ok)]: (status code, [outputs per
    window as replica_oracle's namespace], status[n]).  The buffers start as garbage: the entry must write every
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
    n_ops = np.array([len(o) for o in ops] if n_ops is None else n_ops, np.int32)   # (n_ops: a count the lists cannot express)
    for i, o in enumerate(ops):
        cod[i, :min(len(o), kk)] = np.asarray(o, np.int32)[:kk]
    pod = np.full((n, kk, mm), -7, np.int32)
    cnt, tot, mx = (np.full((n, kk, mm, 2), -7, np.int64) for _ in range(3))
    cn, live, every, place = (np.full((n, kk), -7, np.int32) for _ in range(4))
    own, total = np.full((n, kk, 2, 3), -7, np.int64), np.full((n, kk, 2, 3), -7, np.int64)
    status = np.full(n, -7, np.int32)
    code = what if isinstance(what, int) else lc.WHAT[what]
    rc = _lib.load().mr_windows_replicas(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                         ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m, code, ptr(pod, C.c_int32),
                                         ptr(cnt, C.c_int64), ptr(tot, C.c_int64), ptr(mx, C.c_int64), ptr(cn, C.c_int32),
                                         ptr(live, C.c_int32), ptr(every, C.c_int32), ptr(place, C.c_int32),
                                         ptr(own, C.c_int64), ptr(total, C.c_int64), ptr(status, C.c_int32))
    if check:
        ctx.check(rc, "mr_windows_replicas")
    res = [types.SimpleNamespace(pod=pod[i], cnt=cnt[i], sum=tot[i], max=mx[i], n=cn[i], live=live[i], all=every[i],
                                 place=place[i], own=own[i], tot=total[i]) for i in range(n)]
    return rc, res, status
