"""Helpers of the latency-evidence tests (mr_op_latency / mr_windows_latency, csrc/mr_latency.hip):
the numpy oracle -- exactly the semantics of include/microrank_hip.h -- and the case builders."""
import ctypes as C

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
METHODS = {"linear": 0, "lower": 1, "higher": 2}
WHAT = {"duration": 0, "self": 1}
QS = [0, 0.25, 1 / 3, 0.5, 0.9, 0.99, 0.999, 1]
EDGE_COUNTS = {0, 1, 2, 3, 5, 100, 101}
MIN5 = 5 * 60 * 10**9


def child_sums(table):
    """csum[c] = sum of duration[j] over ALL rows j with parent[j] == c (int64, wrapping)."""
    n = int(max(table.span.max(initial=-1), table.parent.max(initial=-1))) + 1
    csum = np.zeros(max(n, 1), np.int64)
    m = table.parent >= 0
    np.add.at(csum, table.parent[m], table.duration[m].astype(np.int64))
    return csum


def values(table, what):
    d = table.duration.astype(np.int64)
    return d - child_sums(table)[table.span] if what == "self" else d


def in_window(table, t0, t1):
    if t0 == I64_MIN and t1 == I64_MAX:
        return np.ones(table.n_spans, bool)
    return (table.tstart >= t0) & (table.tend <= t1)


def latency_oracle(table, state, t0, t1, podops, what, qs, method):
    """(out[n_ops, 2, n_q], count[n_ops, 2]): per asked op and side (0 normal, 1 abnormal) the count
    of the selected rows and np.quantile of their values; 0.0 for a count of 0."""
    v = values(table, what)
    inside = in_window(table, t0, t1)
    st = np.asarray(state)[table.trace]
    out = np.zeros((len(podops), 2, len(qs)))
    cnt = np.zeros((len(podops), 2), np.int64)
    for j, p in enumerate(podops):
        for side in (0, 1):
            a = v[inside & (table.podop == p) & (st == side + 1)]
            cnt[j, side] = a.size
            if a.size:
                out[j, side] = np.quantile(a, qs, method=method)
    return out, cnt


def hexes(a):
    return [float(x).hex() for x in np.asarray(a, np.float64).reshape(-1)]


# ---------------------------------------------------------------------------------- case builders
def slo_and_state(normal, abnormal, t0=None, t1=None):
    """(a3, ok, state, t0, t1): the SLO of the normal table (oracle.operation_slo) as arrays over the
    abnormal table's service-op codes, and oracle.detect's partition of the abnormal table in
    [t0, t1] (default: the whole table's time range) as mr_detect's state[]."""
    import oracle as orc

    slo = orc.operation_slo(normal.svcop, normal.duration, normal.svcop_names, list(normal.svcop_names))
    a3 = np.zeros(abnormal.n_svcops)
    ok = np.zeros(abnormal.n_svcops, np.uint8)
    for code, name in enumerate(abnormal.svcop_names):
        if name in slo:
            a3[code] = slo[name][0] + 3 * slo[name][1]
            ok[code] = 1
    t0 = int(abnormal.tstart.min()) if t0 is None else t0
    t1 = int(abnormal.tend.max()) if t1 is None else t1
    state = np.zeros(abnormal.n_traces, np.uint8)
    res = orc.detect(abnormal.trace, abnormal.svcop, abnormal.duration, abnormal.tstart, abnormal.tend, t0, t1,
                     {i: float(a3[i]) for i in range(a3.size) if ok[i]})
    if res is not None:
        state[np.asarray(res[2], np.int64)] = 1
        state[np.asarray(res[1], np.int64)] = 2
    return a3, ok, state, t0, t1


def detector_ties(abnormal, a3, ok, t0, t1):
    """Traces of the window whose max(duration) / 1000 equals the detector's expectation exactly."""
    ties = 0
    m = in_window(abnormal, t0, t1)
    for t in np.unique(abnormal.trace[m]):
        rows = m & (abnormal.trace == t)
        ops, cn = np.unique(abnormal.svcop[rows], return_counts=True)
        expect = 0.0
        for o, c in zip(ops, cn):
            if ok[o]:
                expect = expect + float(c) * float(a3[o])
        ties += float(abnormal.duration[rows].max()) / 1000.0 == expect
    return ties


def fault_case(**kw):
    from microrank_amd import synth

    topo, normal, abnormal = synth.window_pair(40, 2000, 3, **kw)
    return topo, normal, abnormal


def quiet_case():
    """window_pair(60, 600, 5): the detector finds no abnormal trace."""
    from microrank_amd import synth

    return synth.window_pair(60, 600, 5)


def edge_table():
    """(table, state, asked ops): ~1,000 rows whose per-(asked op, side) row counts are exactly
    EDGE_COUNTS; op 0 has no row at all; traces of state 0 hold rows of every asked op, which must not
    count; parents inside a trace and a few shared spanID codes, so self time differs from duration."""
    from microrank_amd.spans import SpanTable

    rng = np.random.default_rng(21)
    n_traces, n_ops = 60, 9
    state = (np.arange(n_traces) % 3).astype(np.uint8)
    want = {1: (0, 1), 2: (2, 3), 3: (5, 100), 4: (101, 0), 5: (1, 2)}   # op: (normal, abnormal) rows
    tr, op = [], []
    for o, sides in want.items():
        for side, n in enumerate(sides):
            tr.append(rng.choice(np.flatnonzero(state == side + 1), n))
            op.append(np.full(n, o))
        tr.append(rng.choice(np.flatnonzero(state == 0), 20))   # rows that must not count
        op.append(np.full(20, o))
    n_fill = 1000 - sum(a.size for a in tr)
    tr.append(rng.integers(0, n_traces, n_fill))
    op.append(rng.integers(6, n_ops, n_fill))
    tr, op = np.concatenate(tr), np.concatenate(op)
    order = np.lexsort((rng.random(tr.size), tr))   # a trace's rows adjacent, as a DataFrame has them
    tr, op = tr[order].astype(np.int32), op[order].astype(np.int32)
    S = tr.size
    span = np.arange(S, dtype=np.int64)
    parent = np.full(S, -1, np.int64)
    first = np.searchsorted(tr, tr)   # first row of the row's trace
    has = (np.arange(S) > first) & (rng.random(S) < 0.8)
    parent[has] = rng.integers(first[has], np.arange(S)[has])
    a, b = rng.integers(0, S, 8), rng.integers(0, S, 8)
    span[a] = span[b]                  # shared spanID codes (T11)
    dur = (rng.lognormal(8.0, 1.5, S) + rng.integers(0, 1000, S)).astype(np.int64)
    names = [f"pod_op{o:02d}" for o in range(n_ops)]
    table = SpanTable(tr, op, op.copy(), span, parent, dur, None, None, [f"t{i:04d}" for i in range(n_traces)], names,
                      list(names))
    return table, state, np.array([0, 1, 2, 3, 4, 5], np.int32)


def skewed_table():
    """70,001 rows, 300 pod-ops (test_gpu_slo_quantiles._skewed's shape): op 5 holds 20,000 rows, op 7
    fifty rows of one single value (no parent, no child: self time = duration), four rows per trace
    chained by parents."""
    from microrank_amd.spans import SpanTable

    S, n_ops = 70_001, 300
    rng = np.random.default_rng(70_001)
    sizes = np.ones(n_ops, np.int64)
    sizes[5], sizes[7] = 20_000, 50
    others = np.array([o for o in range(1, n_ops) if o not in (5, 7)])
    w = 1.0 / (1.0 + np.arange(others.size))
    sizes[others] += rng.multinomial(S - int(sizes.sum()), w / w.sum())
    op = np.repeat(np.arange(n_ops), sizes)
    rng.shuffle(op)
    dur = (rng.lognormal(8.0, 1.5, S) + rng.integers(0, 1000, S)).astype(np.int64)
    dur[op == 7] = 12345
    rows = np.arange(S)
    parent = np.where(rows % 4 == 0, -1, rows - 1).astype(np.int64)
    lone = op == 7
    parent[lone] = -1                                # the single-valued op: no parent ...
    nxt = np.flatnonzero(lone[:-1]) + 1
    parent[nxt] = -1                                 # ... and no child
    names = [f"pod_op{o:03d}" for o in range(n_ops)]
    n_traces = (S + 3) // 4
    table = SpanTable((rows // 4).astype(np.int32), op.astype(np.int32), op.astype(np.int32), rows.astype(np.int64), parent,
                      dur, None, None, [f"t{i:06d}" for i in range(n_traces)], names, list(names))
    state = rng.integers(0, 3, n_traces).astype(np.uint8)
    return table, state, sizes


def banded_table(times=True):
    """test_gpu_slo_quantiles._banded's shape over pod-ops: three bands of rows around the window
    [10_000, 20_000], rows exactly on each bound and rows one tick over; ops 10 and 11 only outside."""
    from microrank_amd.spans import SpanTable

    rng = np.random.default_rng(3)
    t0, t1 = 10_000, 20_000
    n = 900
    op = rng.integers(0, 10, 3 * n)
    ts = np.concatenate([rng.integers(1_000, 5_000, n), rng.integers(t0, 15_000, n), rng.integers(20_001, 30_000, n)])
    te = np.concatenate([ts[:n] + rng.integers(0, 4_999, n), ts[n:2 * n] + rng.integers(0, 5_000, n),
                         ts[2 * n:] + rng.integers(0, 5_000, n)])
    ts[n:n + 4], te[n:n + 4] = [t0, t0, 15_000, t0], [t0, t1, t1, 12_000]
    ts[n + 4:n + 8], te[n + 4:n + 8] = [t0 - 1, 15_000, t0 - 1, t0], [15_000, t1 + 1, t1 + 1, t1 + 1]
    op[:40], op[2 * n:2 * n + 40] = 10, 11
    op[n + 4:n + 8] = [10, 11, 10, 11]
    dur = (rng.lognormal(8.0, 1.5, 3 * n) + rng.integers(0, 1000, 3 * n)).astype(np.int64)
    order = rng.permutation(3 * n)
    op, dur, ts, te = op[order].astype(np.int32), dur[order], ts[order].astype(np.int64), te[order].astype(np.int64)
    S = op.size
    rows = np.arange(S)
    parent = np.where(rows % 4 == 0, -1, rows - 1).astype(np.int64)
    names = [f"pod_op{o:02d}" for o in range(12)]
    n_traces = (S + 3) // 4
    table = SpanTable((rows // 4).astype(np.int32), op, op.copy(), rows.astype(np.int64), parent, dur,
                      ts if times else None, te if times else None, [f"t{i:05d}" for i in range(n_traces)], names,
                      list(names))
    state = rng.integers(0, 3, n_traces).astype(np.uint8)
    return table, state, t0, t1


# ---------------------------------------------------------------------------------- GPU callers
def op_latency_call(ctx, dev, state, podops, what, qs, method=0, t0=I64_MIN, t1=I64_MAX, n_ops=None, n_q=None):
    """(status, out[n_ops, 2, n_q], count[n_ops, 2]) of one mr_op_latency call."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    qv = np.ascontiguousarray(np.asarray(qs, np.float64).reshape(-1))
    cod = np.ascontiguousarray(podops, np.int32)
    st = np.ascontiguousarray(state, np.uint8)
    out = np.full((max(cod.size, 1), 2, max(qv.size, 1)), -7.0)
    cnt = np.full((max(cod.size, 1), 2), -7, np.int64)
    rc = _lib.load().mr_op_latency(ctx.h, dev.h, t0, t1, ptr(st, C.c_uint8), ptr(cod, C.c_int32),
                                   cod.size if n_ops is None else n_ops, what, ptr(qv, C.c_double),
                                   qv.size if n_q is None else n_q, method, ptr(out, C.c_double), ptr(cnt, C.c_int64))
    return rc, out, cnt


def last_error(ctx):
    from microrank_amd import _lib

    m = _lib.load().mr_last_error(ctx.h)
    return m.decode() if m else ""


def check_op_latency(ctx, dev, table, state, podops, qs=QS, t0=I64_MIN, t1=I64_MAX, whats=("duration", "self"),
                     methods=("linear", "lower", "higher")):
    """Every asked method and value against the numpy oracle, float.hex for float.hex; returns the
    counts of the last call."""
    from microrank_amd import _lib

    cnt = None
    for what in whats:
        for name in methods:
            rc, out, cnt = op_latency_call(ctx, dev, state, podops, WHAT[what], qs, METHODS[name], t0, t1)
            assert rc == _lib.MR_OK, (what, name, last_error(ctx))
            eo, ec = latency_oracle(table, state, t0, t1, podops, what, qs, name)
            assert cnt.tolist() == ec.tolist(), (what, name)
            assert hexes(out) == hexes(eo), (what, name)
    return cnt
