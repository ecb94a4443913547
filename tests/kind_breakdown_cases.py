"""Helpers of the kind-breakdown tests (mr_windows_kind_breakdown, csrc/mr_kind_breakdown.hip): the numpy
oracle -- exactly the semantics of include/microrank_hip.h, from the span table's rows and a detector
partition (oracle.detect's lists as mr_detect's state[]) -- and the case builders.  Everything cached
here is shared between tests and read-only."""
import ctypes as C
import functools
import types

import numpy as np

WINDOWS = ("ties", "mid", "ragged", "one_trace")
MS = (1, 8, 32)
K_TOP = 11
BOUNDARY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 3000)


def trace_kinds(table):
    """(kind id per trace code (-1: a trace without rows), rows per trace, distinct pod-ops per trace,
    op sets by kind id).  A kind: the sorted set of distinct pod-op codes over all rows of the trace and
    the bits of float32(1.0 / rows)."""
    nt = table.n_traces
    rows = np.bincount(table.trace, minlength=nt)
    pairs = np.unique(np.stack([table.trace.astype(np.int64), table.podop.astype(np.int64)], 1), axis=0)
    first = np.searchsorted(pairs[:, 0], np.arange(nt + 1))
    ids, kid, opsets = {}, np.full(nt, -1, np.int64), []
    nops = np.diff(first)
    for t in range(nt):
        if rows[t] == 0:
            continue
        ops = tuple(pairs[first[t]:first[t + 1], 1].tolist())
        key = (ops, int(np.float32(1.0 / float(rows[t])).view(np.uint32)))
        if key not in ids:
            ids[key] = len(ids)
            opsets.append(frozenset(ops))
        kid[t] = ids[key]
    return kid, rows, nops, opsets


def live_kinds(table, state, kinds=None):
    """[(n_abn, n_nor, rep, spans, ops, op set)] of the window's live kinds, in no particular order."""
    kid, rows, nops, opsets = kinds if kinds is not None else trace_kinds(table)
    state = np.asarray(state)
    out = {}
    for t in np.flatnonzero((state == 1) | (state == 2)).tolist():   # (ascending codes)
        k = int(kid[t])
        e = out.setdefault(k, [0, 0, -1, -1])
        if state[t] == 2:
            e[0] += 1
            if e[2] < 0:
                e[2] = t
        else:
            e[1] += 1
            if e[3] < 0:
                e[3] = t
    res = []
    for k, (na, nn, fa, fn) in out.items():
        rep = fa if na else fn
        res.append((na, nn, rep, int(rows[rep]), int(nops[rep]), opsets[k]))
    return res


def breakdown_oracle(table, state, asked, k, m, kinds=None):
    """The nine outputs of one window as the C entry lays them out for K = k: trace / abn / nor / spans /
    ops [k, m], n / kinds [k], tot [k, 2]; asked: codes, -1 for every kind.  state None: an empty
    window (the padding)."""
    col = [np.full((k, m), -1, np.int32)] + [np.zeros((k, m), np.int32) for _ in range(4)]
    n, nk, tot = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros((k, 2), np.int64)
    if state is not None:
        live = live_kinds(table, state, kinds)
        for j, p in enumerate(asked):
            sel = [e for e in live if p == -1 or p in e[5]]
            sel.sort(key=lambda e: (-e[0], e[1], e[2]))
            nk[j] = len(sel)
            tot[j] = [sum(e[0] for e in sel), sum(e[1] for e in sel)]
            n[j] = min(m, len(sel))
            for r, e in enumerate(sel[:m]):
                col[0][j, r], col[1][j, r], col[2][j, r], col[3][j, r], col[4][j, r] = e[2], e[0], e[1], e[3], e[4]
    return types.SimpleNamespace(trace=col[0], abn=col[1], nor=col[2], spans=col[3], ops=col[4], n=n, kinds=nk, tot=tot)


FIELDS = ("trace", "abn", "nor", "spans", "ops", "n", "kinds", "tot")


def same(got, exp):
    """Exact integer equality of every output of a window."""
    for f in FIELDS:
        a, b = getattr(got, f), getattr(exp, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tolist() == b.tolist(), f


def state_of(n_traces, abnormal, normal):
    st = np.zeros(n_traces, np.uint8)
    st[np.asarray(list(normal), np.int64)] = 1
    st[np.asarray(list(abnormal), np.int64)] = 2
    st.setflags(write=False)
    return st


def top_ops(table, state, n=K_TOP):
    """The window's `top list' for the tests: the n pod-ops on the most abnormal traces (ties: the smaller
    code), which need no ranking -- any ops would do."""
    ab = np.asarray(state)[table.trace] == 2
    pairs = np.unique(np.stack([table.trace[ab], table.podop[ab]], 1), axis=0)
    cov = np.bincount(pairs[:, 1], minlength=table.n_podops) if pairs.size else np.zeros(table.n_podops, np.int64)
    order = np.lexsort((np.arange(cov.size), -cov))
    return [int(c) for c in order[:n] if cov[c] > 0]


def absent_op(table, state):
    """A pod-op code with no trace in the window (None: every pod-op has one)."""
    live = np.isin(np.asarray(state)[table.trace], (1, 2))
    gone = np.setdiff1d(np.arange(table.n_podops), table.podop[live])
    return int(gone[0]) if gone.size else None


# ---------------------------------------------------------------------------------- case builders
@functools.lru_cache(maxsize=None)
def window(name):
    """A window of window_exemplar_cases (`ties`, `mid`, `ragged`, `one_trace`) or `fault`
    (latency_cases.fault_case()): table, a3, ok, t0, t1, state (oracle.detect), kinds (trace_kinds)."""
    import latency_cases as lc
    import window_exemplar_cases as wx

    if name == "fault":
        _, normal, abnormal = lc.fault_case()
        a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
        table = abnormal
        state = np.array(state)
        state.setflags(write=False)
    else:
        table, _, c, t0, t1 = wx.table(name)
        a3, ok = np.full(table.n_svcops, c, np.float64), np.ones(table.n_svcops, np.uint8)
        ab, no = wx.detected(name)
        state = state_of(table.n_traces, ab, no)
    return types.SimpleNamespace(name=name, table=table, a3=a3, ok=ok, t0=t0, t1=t1, state=state, kinds=trace_kinds(table))


def asked_ops(w):
    """The asked slots of a window's case: its top list (the ranking oracle's where window_exemplar_cases
    has one, else top_ops), -1, the first top op again, an absent op (where the window has one)."""
    if w.name in WINDOWS:
        import window_exemplar_cases as wx

        top = list(wx.oracle(w.name, 25).top)[:K_TOP - 3]
    else:
        top = top_ops(w.table, w.state, K_TOP - 3)
    ops = top + [-1]
    ops.append(ops[0])
    gone = absent_op(w.table, w.state)
    if gone is not None:
        ops.append(gone)
    return ops


@functools.lru_cache(maxsize=None)
def expected(name, m):
    w = window(name)
    return breakdown_oracle(w.table, w.state, asked_ops(w), K_TOP, m, w.kinds)


def summary(w):
    """The shape figures of a window: traces, live kinds, kinds of more than one member, kinds with
    traces on both sides, the largest kind, the (n_abn, n_nor) pairs in answer order."""
    live = sorted(live_kinds(w.table, w.state, w.kinds), key=lambda e: (-e[0], e[1], e[2]))
    return types.SimpleNamespace(traces=int(np.isin(w.state, (1, 2)).sum()), live=len(live),
                                 multi=sum(e[0] + e[1] > 1 for e in live), both=sum(e[0] > 0 and e[1] > 0 for e in live),
                                 largest=max(e[0] + e[1] for e in live), pairs=[(e[0], e[1]) for e in live])


@functools.lru_cache(maxsize=None)
def boundary():
    """A table of direct arrays whose kinds have exactly BOUNDARY_SIZES members inside the window -- the
    layout's runs end on, before and after every wave (64) and block (256, 1024) boundary and span
    several blocks -- plus one kind of 40 traces wholly outside it.  Kind i: pod-ops {0, i + 1} and, for
    odd i, {i + 20} too, 2 + i % 3 rows per pod-op.  Trace codes are dealt at random, so a kind's
    members are spread over the codes.  One constant SLO a3 = 1.0 (ms) for every service-op: a trace of
    r rows expects r ms, its largest duration is r * 100 (normal) or r * 10_000 (abnormal) duration
    units of 1 us; the first two members of every kind take one side each."""
    from microrank_amd.spans import SpanTable

    rng = np.random.default_rng(2024)
    sizes = list(BOUNDARY_SIZES) + [40]
    nt = sum(sizes)
    codes = rng.permutation(nt)
    t0, t1 = 1_000_000, 2_000_000
    tr, op, dur, ts, te = [], [], [], [], []
    at = 0
    for i, size in enumerate(sizes):
        ops = [0, i + 1] + ([i + 20] if i % 2 else [])
        per = 2 + i % 3
        rows = per * len(ops)
        mine = np.sort(codes[at:at + size])
        at += size
        outside = i == len(sizes) - 1
        abn = rng.random(size) < 0.5
        abn[:2] = [True, False][:size]
        for j, t in enumerate(mine.tolist()):
            tr += [t] * rows
            op += ops * per
            d = rng.integers(1, rows * 100, rows)
            d[rng.integers(0, rows)] = rows * 10_000 if abn[j] else rows * 100
            dur += d.tolist()
            s0 = t1 + 10 if outside else int(rng.integers(t0, t1 - 1000))
            ts += [s0] * rows
            te += [s0 + 500] * rows
    order = np.lexsort((rng.random(len(tr)), np.asarray(tr)))   # a trace's rows adjacent, pod-ops mixed
    tr, op = np.asarray(tr, np.int32)[order], np.asarray(op, np.int32)[order]
    dur, ts, te = np.asarray(dur, np.int64)[order], np.asarray(ts, np.int64)[order], np.asarray(te, np.int64)[order]
    S = tr.size
    n_ops = int(op.max()) + 2                                   # (the last code: a pod-op no row has)
    names = [f"pod_op{o:02d}" for o in range(n_ops)]
    parent = np.where(np.r_[False, tr[1:] == tr[:-1]], np.arange(S) - 1, -1).astype(np.int64)   # a chain per trace
    table = SpanTable(tr, op, op.copy(), np.arange(S, dtype=np.int64), parent, dur, ts, te,
                      [f"t{i:05d}" for i in range(nt)], names, list(names))
    a3, ok = np.ones(n_ops, np.float64), np.ones(n_ops, np.uint8)
    import oracle as orc

    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, t0, t1,
                     {i: 1.0 for i in range(n_ops)})
    state = state_of(nt, res[1], res[2])
    return types.SimpleNamespace(name="boundary", table=table, a3=a3, ok=ok, t0=t0, t1=t1, state=state,
                                 kinds=trace_kinds(table))


@functools.lru_cache(maxsize=None)
def big_window():
    """synth.window_pair(300, 20_000, 7)'s window table (20,000 traces, ~1.08 M rows: more than 20 build
    blocks of the layout, ~18.7k kinds) under window_exemplar_cases' constant-SLO rule: c the median over
    traces of (max duration / 1000 / rows), so about half of the traces are abnormal."""
    import oracle as orc
    from microrank_amd import synth

    _, _, table = synth.window_pair(300, 20_000, 7)
    mx = np.zeros(table.n_traces, np.int64)
    np.maximum.at(mx, table.trace, table.duration)
    rows = np.bincount(table.trace, minlength=table.n_traces)
    c = float(np.median(mx / 1000.0 / rows))
    t0, t1 = int(table.tstart.min()), int(table.tend.max())
    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, t0, t1,
                     {i: c for i in range(table.n_svcops)})
    state = state_of(table.n_traces, res[1], res[2])
    a3, ok = np.full(table.n_svcops, c, np.float64), np.ones(table.n_svcops, np.uint8)
    return types.SimpleNamespace(name="big", table=table, a3=a3, ok=ok, t0=t0, t1=t1, state=state, kinds=trace_kinds(table))


# ---------------------------------------------------------------------------------- GPU caller
def call(ctx, wins, ops, k, m, check=True, n_ops=None):
    """One raw mr_windows_kind_breakdown call over wins = [(DeviceSpans, t0, t1, a3, ok)]: (status code,
    [outputs per window as breakdown_oracle's namespace], status[n]).  The buffers start as garbage: the
    entry must write every word."""
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
    col = [np.full((n, kk, mm), -7, np.int32) for _ in range(5)]
    cnt, kinds = np.full((n, kk), -7, np.int32), np.full((n, kk), -7, np.int32)
    tot = np.full((n, kk, 2), -7, np.int64)
    status = np.full(n, -7, np.int32)
    rc = _lib.load().mr_windows_kind_breakdown(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                               ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, m,
                                               *[ptr(c, C.c_int32) for c in col], ptr(cnt, C.c_int32),
                                               ptr(kinds, C.c_int32), ptr(tot, C.c_int64), ptr(status, C.c_int32))
    if check:
        ctx.check(rc, "mr_windows_kind_breakdown")
    out = [types.SimpleNamespace(trace=col[0][i], abn=col[1][i], nor=col[2][i], spans=col[3][i], ops=col[4][i], n=cnt[i],
                                 kinds=kinds[i], tot=tot[i]) for i in range(n)]
    return rc, out, status


def raw_bytes(out):
    return b"".join(getattr(o, f).tobytes() for o in out for f in FIELDS)
