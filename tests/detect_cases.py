"""Helpers of the detector edge tests (mr_detect, mr_detect_sweep, the detectors fused into the window
builds, and the per-trace scalars of mr_span_index.hip they all read): the oracles -- oracle.detect's
lists as mr_detect's state[], plain numpy counts of in-window rows -- and the case builders.  Tables are
built directly from arrays, times are small integers (some negative), and the detector takes a3 / a3_valid
arrays.  Everything cached here is shared between tests and read-only."""
import ctypes as C
import functools
import math
import types
from fractions import Fraction

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
WAVE, BLOCK = 64, 256            # k_ix_trace_stats / k_win_keys: lanes per wave, rows per block
DB, STAGE = 256, 4096            # detect_block: traces per block, staged (trace, service-op) entries


def make_table(trace, svcop, dur, ts=None, te=None, *, podop=None, span=None, parent=None, n_traces=None,
               n_svcops=None, n_podops=None):
    """A SpanTable from arrays; pod-op defaults to svcop % 5, every span a root with its own spanID."""
    from microrank_amd.spans import SpanTable

    trace, svcop = np.asarray(trace, np.int32), np.asarray(svcop, np.int32)
    S = trace.size
    podop = (svcop % 5).astype(np.int32) if podop is None else np.asarray(podop, np.int32)
    span = np.arange(S, dtype=np.int64) if span is None else np.asarray(span, np.int64)
    parent = np.full(S, -1, np.int64) if parent is None else np.asarray(parent, np.int64)
    nt = int(trace.max()) + 1 if n_traces is None else n_traces
    ns = int(svcop.max()) + 1 if n_svcops is None else n_svcops
    npo = int(podop.max()) + 1 if n_podops is None else n_podops
    pick = lambda a: None if a is None else np.asarray(a, np.int64)
    return SpanTable(trace, podop, svcop, span, parent, np.asarray(dur, np.int64), pick(ts), pick(te),
                     [f"t{i:05d}" for i in range(nt)], [f"pod_op{i:05d}" for i in range(npo)],
                     [f"svc_op{i:05d}" for i in range(ns)])


def per_span(table, seed=1):
    """The table with times that differ inside its traces (the row-level route: uniform_times false): each
    row's start moved forward and its end back by 0..2 (the tables given here have ends at least 4 after
    their starts), so a window that holds a trace whole holds each of its rows."""
    rng = np.random.default_rng(seed)
    S = table.n_spans
    d0, d1 = rng.integers(0, 3, S), rng.integers(0, 3, S)
    sizes = np.bincount(table.trace)
    if sizes.max() > 1:   # one trace's times differ for certain
        r = np.flatnonzero(table.trace == int(np.argmax(sizes > 1)))
        d0[r[0]], d0[r[1]] = 0, 2
    out = table.take(np.arange(S))
    out.tstart, out.tend = table.tstart + d0, table.tend - d1
    return out


def uniform_times(table):
    """Whether start and end are constant inside every trace (what the index checks)."""
    for a in (table.tstart, table.tend):
        lo, hi = np.full(table.n_traces, I64_MAX), np.full(table.n_traces, I64_MIN)
        np.minimum.at(lo, table.trace, a)
        np.maximum.at(hi, table.trace, a)
        if (lo[hi >= lo] != hi[hi >= lo]).any():
            return False
    return True


# ---------------------------------------------------------------------------------- the oracles
def slo_dict(a3, ok):
    return {i: float(a3[i]) for i in range(len(a3)) if ok[i]}


def detect_oracle(table, t0, t1, a3, ok):
    """(state[n_traces] or None for an empty window, n_abnormal, n_normal, in-window rows): oracle.detect's
    lists as mr_detect's state[], and a numpy count of the rows with tstart >= t0 and tend <= t1."""
    import oracle as orc

    rows = int(((table.tstart >= t0) & (table.tend <= t1)).sum())
    res = orc.detect(table.trace, table.svcop, table.duration, table.tstart, table.tend, t0, t1, slo_dict(a3, ok))
    if res is None:
        assert rows == 0
        return None, 0, 0, 0
    state = np.zeros(table.n_traces, np.uint8)
    state[np.asarray(res[2], np.int64)] = 1
    state[np.asarray(res[1], np.int64)] = 2
    return state, len(res[1]), len(res[2]), rows


def trace_rows(table):
    return np.bincount(table.trace, minlength=table.n_traces).astype(np.int64)


def sweep_oracle(table, a3, ok, t_begin, grain, window, n_win):
    """(state, n_abnormal[n_win], n_normal[n_win], n_rows[n_win] int64) of mr_detect_sweep: the partition
    of the whole table (times are constant inside a trace, so it does not depend on the window), and per
    window m the mask (ts >= t_begin + m*grain) & (te <= t_begin + m*grain + window) over the rows."""
    state, _, _, _ = detect_oracle(table, I64_MIN, I64_MAX, a3, ok)
    na, nn, rows = np.zeros(n_win, np.int32), np.zeros(n_win, np.int32), np.zeros(n_win, np.int64)
    st_row = state[table.trace]
    for m0 in range(0, n_win, 512):
        p = t_begin + grain * np.arange(m0, min(m0 + 512, n_win), dtype=np.int64)[:, None]
        mask = (table.tstart[None, :] >= p) & (table.tend[None, :] <= p + window)
        rows[m0:m0 + 512] = mask.sum(1)
        for out, s in ((na, 2), (nn, 1)):
            hit = np.zeros((mask.shape[0], table.n_traces), bool)
            w, r = np.nonzero(mask & (st_row == s)[None, :])
            hit[w, table.trace[r]] = True
            out[m0:m0 + 512] = hit.sum(1)
    return state, na, nn, rows


def fl(x):
    """A Fraction rounded to the nearest double (ties to even), as one IEEE operation rounds."""
    return float(Fraction(x))


def expect_exact(terms, mode="seq"):
    """The detector's expect over terms [(count, a3), ...] in the given order, every operation modelled with
    fractions.Fraction and rounded once: `seq` rounds each product and each add (the reference's and the
    kernels' arithmetic), `fused` rounds product-and-add together (a contracted multiply-add), `reverse` is
    `seq` over the terms from last to first -- fl(p1 + fl(p2 + p3)) for three terms."""
    e = 0.0
    for c, a in (reversed(terms) if mode == "reverse" else terms):
        if mode == "fused":
            e = fl(Fraction(e) + Fraction(c) * Fraction(a))
        else:
            e = fl(Fraction(e) + Fraction(fl(Fraction(c) * Fraction(a))))
    return e


def real_of(mx):
    return fl(Fraction(fl(Fraction(int(mx)))) / Fraction(1000.0))


# ---------------------------------------------------------------------------------- A: row order
ORDER_SIZES = (1, 2, 63, 64, 65, 300)
ORDERS = ("grouped", "alternating", "round_robin", "random", "by_time")
ORDER_NT, ORDER_OPS = 40, 9
ORDER_CUT = (0, 1000)


@functools.lru_cache(maxsize=None)
def order_base():
    """The logical table of part A, rows grouped by trace: 40 traces of 1, 2, 63, 64, 65, 300 and 8..47
    rows, 9 service-ops (op 8 has no SLO and an a3 of 1e300), 18 pod-ops, parents inside a trace; about half
    the traces hold one row above 1.5 x their expect, two traces hold no positive duration."""
    rng = np.random.default_rng(4101)
    sizes = np.concatenate([ORDER_SIZES, rng.integers(8, 48, ORDER_NT - len(ORDER_SIZES))])
    sizes = sizes[rng.permutation(ORDER_NT)]
    trace = np.repeat(np.arange(ORDER_NT), sizes)
    S = trace.size
    svcop = rng.integers(0, ORDER_OPS, S)
    podop = svcop * 2 + rng.integers(0, 2, S)
    rows = np.arange(S)
    first = np.searchsorted(trace, trace)
    has = (rows > first) & (rng.random(S) < 0.8)
    parent = np.full(S, -1, np.int64)
    parent[has] = rng.integers(first[has], rows[has])   # the spanID (= logical row) of an earlier row of the trace
    a3 = np.round(rng.uniform(0.5, 20.0, ORDER_OPS), 4)
    ok = np.ones(ORDER_OPS, np.uint8)
    a3[8], ok[8] = 1e300, 0
    dur = rng.integers(-20, 400, S)
    small = [t for t in range(ORDER_NT) if 8 <= sizes[t] < 48]
    dropped = small[1::7][:2]
    for t in range(ORDER_NT):
        r = np.flatnonzero(trace == t)
        if t in dropped:
            dur[r] = -rng.integers(0, 5, r.size)
        elif t % 2 == 0:
            dur[rng.choice(r)] = int(1500 * float((a3[svcop[r]] * ok[svcop[r]]).sum())) + 1
    tts = rng.integers(-400, 1400, ORDER_NT)
    tte = tts + rng.integers(0, 300, ORDER_NT)
    rts = tts[trace] + rng.integers(-60, 60, S)
    rte = rts + rng.integers(0, 120, S)
    return types.SimpleNamespace(sizes=sizes, trace=trace, svcop=svcop, podop=podop, span=rows.astype(np.int64),
                                 parent=parent, dur=dur, a3=a3, ok=ok, tts=tts, tte=tte, rts=rts, rte=rte,
                                 dropped=dropped)


@functools.lru_cache(maxsize=None)
def order_perm(name):
    """Stored row -> logical row of one of ORDERS."""
    b = order_base()
    S = b.trace.size
    first = np.searchsorted(b.trace, b.trace)
    if name == "grouped":
        return np.arange(S)
    if name == "alternating":   # the 300-row and the 65-row trace, A B A B ..., in front; then the rest
        ra = np.flatnonzero(b.trace == int(np.flatnonzero(b.sizes == 300)[0]))
        rb = np.flatnonzero(b.trace == int(np.flatnonzero(b.sizes == 65)[0]))
        head = np.stack([ra[:65], rb]).T.reshape(-1)
        rest = np.setdiff1d(np.arange(S), np.concatenate([ra, rb]))
        return np.concatenate([head, ra[65:], rest])
    if name == "round_robin":   # every trace's k-th row, k = 0, 1, ...
        return np.lexsort((b.trace, np.arange(S) - first))
    if name == "random":
        return np.random.default_rng(7).permutation(S)
    if name == "by_time":
        return np.argsort(b.rts, kind="stable")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def order_table(name, uniform):
    """Part A's table in one stored order; uniform: trace-level times, else a start and end per span."""
    b, p = order_base(), order_perm(name)
    ts, te = (b.tts[b.trace], b.tte[b.trace]) if uniform else (b.rts, b.rte)
    return make_table(b.trace[p], b.svcop[p], b.dur[p], ts[p], te[p], podop=b.podop[p], span=b.span[p],
                      parent=b.parent[p], n_traces=ORDER_NT, n_svcops=ORDER_OPS, n_podops=2 * ORDER_OPS)


def order_windows(table):
    """(a window that holds every row, one that cuts the table)."""
    return (int(table.tstart.min()), int(table.tend.max())), ORDER_CUT


def interleaving(trace):
    """(a trace has rows on both sides of a wave edge, of a block edge, a trace has two rows inside one
    wave with another trace's row between them)."""
    trace = np.asarray(trace)
    S = trace.size
    out = []
    for edge in (WAVE, BLOCK):
        found = False
        for k in range(edge, S, edge):
            found = found or bool(np.intersect1d(trace[:k], trace[k:]).size)
        out.append(found)
    sand = False
    for w0 in range(0, S, WAVE):
        w = trace[w0:w0 + WAVE]
        for t in np.unique(w):
            pos = np.flatnonzero(w == t)
            sand = sand or bool(pos.size and pos[-1] - pos[0] + 1 > pos.size)
    return out[0], out[1], sand


BASE_NS = 10**15


@functools.lru_cache(maxsize=None)
def append_case():
    """Part A's rows in start-time order as a reference-schema frame (trace-level times) cut in two chunks
    in the middle of the frame, and a keep_from that retires some traces of the first chunk:
    (chunk 1, chunk 2, keep_from ns, {svcop name: (a3, valid)})."""
    import pandas as pd

    b, p = order_base(), order_perm("by_time")
    tr, op, pod = b.trace[p], b.svcop[p], b.podop[p] % 2
    df = pd.DataFrame({
        "traceID": [f"t{t:03d}" for t in tr],
        "spanID": [f"s{s:05d}" for s in b.span[p]],
        "ParentSpanId": [f"s{q:05d}" if q >= 0 else None for q in b.parent[p]],
        "serviceName": [f"svc{o:02d}" for o in op],
        "operationName": ["op"] * tr.size,
        "podName": [f"svc{o:02d}-pod{k}" for o, k in zip(op, pod)],
        "duration": b.dur[p].astype(np.int64),
        "startTime": pd.to_datetime(BASE_NS + b.tts[tr]),
        "endTime": pd.to_datetime(BASE_NS + b.tte[tr]),
    })
    half = tr.size // 2
    slo = {f"svc{o:02d}_op": (float(b.a3[o]), int(b.ok[o])) for o in range(ORDER_OPS)}
    return df.iloc[:half].reset_index(drop=True), df.iloc[half:].reset_index(drop=True), BASE_NS + 100, slo


def slo_by_name(table, slo):
    a3 = np.array([slo[n][0] for n in table.svcop_names])
    ok = np.array([slo[n][1] for n in table.svcop_names], np.uint8)
    return a3, ok


# ---------------------------------------------------------------------------------- B: verdict arithmetic
N_SEARCH = 100   # stored cases of each searched kind


@functools.lru_cache(maxsize=None)
def searched_cases():
    """{'fma': [...], 'order': [...]}: cases (mx, [(count, a3), ...]) from a seeded search.  mx in
    1000..5*10^6, counts in 1..9, every a3 a 4-decimal number, the first solved so that the decimal sum is
    mx / 1000 exactly: the doubles then land within an ulp of real, and the rounding decides.
    fma: two ops, the sequential sum and the fused one on opposite sides of real.
    order: three or four ops, the left-to-right sum and the right-to-left one on opposite sides."""
    rng = np.random.default_rng(20240)
    out = {"fma": [], "order": []}
    draws = 0
    while min(len(v) for v in out.values()) < N_SEARCH and draws < 400_000:
        draws += 1
        kind = "fma" if draws % 2 else "order"
        k = 2 if kind == "fma" else int(rng.integers(3, 5))
        mx = int(rng.integers(1000, 5_000_001))
        cn = [int(c) for c in rng.integers(1, 10, k)]
        target = mx * 10                     # in units of 1e-4
        A = [0] + [int(rng.integers(1, max(2, target // (k * c)))) for c in cn[1:]]
        rem = target - sum(c * x for c, x in zip(cn[1:], A[1:]))
        if rem <= 0 or rem % cn[0]:
            continue
        A[0] = rem // cn[0]
        terms = [(c, x / 10000.0) for c, x in zip(cn, A)]
        real = mx / 1000.0
        seq = 0.0
        for c, a in terms:
            seq = seq + float(c) * a
        other = expect_exact(terms, "fused" if kind == "fma" else "reverse")
        if (real > seq) != (real > other) and len(out[kind]) < N_SEARCH:
            out[kind].append((mx, terms))
    out["draws"] = draws
    return out


def _edge_cases():
    """[(kind, name, mx or explicit durations, [(count, a3, valid), ...])]: the hand-made traces of part B."""
    up, dn = (lambda x: math.nextafter(x, math.inf)), (lambda x: math.nextafter(x, -math.inf))
    cases = []
    tie_mx = [1, 7, 1000, 1211063, 4999999, 123457] + np.random.default_rng(12).integers(2, 5_000_000, 14).tolist()
    for i, mx in enumerate(tie_mx):   # max / 1000.0 == expect: normal
        r = mx / 1000.0
        cases += [("ties", f"tie{i}", mx, [(1, r, 1)]), ("ties", f"below{i}", mx, [(1, dn(r), 1)]),
                  ("ties", f"above{i}", mx, [(1, up(r), 1)])]
    cases += [("signs", "max0", [0, 0, -3], [(3, 0.001, 1)]),
              ("signs", "max_neg", [-5, -9], [(2, 0.001, 1)]),
              ("signs", "pos_beside_neg", [-7, 9, -1000, -1], [(4, 0.002, 1)]),       # 0.009 > 0.008
              ("signs", "pos_beside_neg_n", [-7, 8, -1000, -1], [(4, 0.002, 1)]),     # 0.008 == 0.008
              ("signs", "max1_tie", 1, [(1, 0.001, 1)]),
              ("signs", "max1_below", 1, [(1, dn(0.001), 1)])]
    r = 2500 / 1000.0
    cases += [("valid", "nan_skipped", 2500, [(1, dn(r), 1), (2, math.nan, 0)]),       # abnormal, unless NaN is added
              ("valid", "huge_skipped", 2500, [(3, 1e300, 0), (1, dn(r), 1)]),
              ("valid", "neg_huge_skipped", 2500, [(1, r, 1), (1, -1e300, 0)]),            # normal, unless -1e300 is added
              ("valid", "none_valid_pos", 1, [(2, math.nan, 0), (1, 1e300, 0)]),       # expect +0.0: abnormal
              ("valid", "none_valid_zero", [0, 0], [(2, 5.0, 0)]),                     # dropped
              ("valid", "neg_a3_tie", 2500, [(2, -2.5, 1), (1, 7.5, 1)]),              # 2.5 == 2.5: normal
              ("valid", "neg_a3_over", 2501, [(2, -2.5, 1), (1, 7.5, 1)]),
              ("valid", "neg_expect", 1, [(3, -2.5, 1)])]
    for i, (n, a, mx) in enumerate(((3000, 0.1, 300_000), (2999, 0.3, 899_700), (1500, 0.7, 1_050_000))):
        cases += [("big", f"big{i}", mx, [(n, a, 1)]), ("big", f"big{i}_over", mx + 1, [(n, a, 1)])]   # one op, many rows
    return cases


def _mx_for(real_target):
    """The integer max duration whose / 1000.0 is the smallest real >= real_target."""
    mx = int(math.floor(real_target * 1000.0))
    while mx / 1000.0 < real_target:
        mx += 1
    return mx


VERDICT_KINDS = ("ties", "signs", "valid", "big", "fma", "order")


@functools.lru_cache(maxsize=None)
def verdict_case():
    """Part B's table: one trace per case, every case its own service-ops (codes ascending in the order of
    its terms), trace k alone in the time slot [10 * k - 1000, + 4], a kind's traces in adjacent slots.
    Returns a namespace: table (uniform times), a3, ok, names, kind windows {kind: (t0, t1)}, terms per
    trace."""
    cases = list(_edge_cases())
    found = searched_cases()
    for kind in ("fma", "order"):
        for i, (mx, terms) in enumerate(found[kind]):
            cases.append((kind, f"{kind}{i}", mx, [(c, a, 1) for c, a in terms]))
    cases.sort(key=lambda c: VERDICT_KINDS.index(c[0]))
    rng = np.random.default_rng(5)
    tr, op, du, a3, ok, names, kinds, terms = [], [], [], [], [], [], [], []
    for t, (kind, name, mx, ops) in enumerate(cases):
        n = sum(c for c, _, _ in ops)
        if isinstance(mx, list):
            d = np.array(mx, np.int64)
            assert d.size == n
        else:   # the max once or twice, the other rows below it
            d = mx - rng.integers(0, 4, n)
            d[rng.integers(0, n)] = mx
        codes = np.concatenate([np.full(c, len(a3) + j) for j, (c, _, _) in enumerate(ops)])
        codes = codes[rng.permutation(n)]   # (row order inside a trace must not matter)
        tr.append(np.full(n, t))
        op.append(codes)
        du.append(d)
        a3 += [a for _, a, _ in ops]
        ok += [v for _, _, v in ops]
        names.append(name)
        kinds.append(kind)
        terms.append(ops)
    tr, op, du = np.concatenate(tr), np.concatenate(op), np.concatenate(du)
    slot = 10 * tr.astype(np.int64) - 1000
    table = make_table(tr, op, du, slot, slot + 4, podop=op % 7, n_traces=len(cases), n_svcops=len(a3))
    kinds = np.array(kinds)
    windows = {k: (10 * int(np.flatnonzero(kinds == k)[0]) - 1000, 10 * int(np.flatnonzero(kinds == k)[-1]) - 996)
               for k in VERDICT_KINDS}
    return types.SimpleNamespace(table=table, a3=np.array(a3), ok=np.array(ok, np.uint8), names=names, kinds=kinds,
                                 windows=windows, terms=terms)


# ---------------------------------------------------------------------------------- C: window edges
EDGE_WIN = (-10, 25)


@functools.lru_cache(maxsize=None)
def edge_uniform():
    """(table, a3, ok, inside[n_traces]): trace-level times on and one tick outside the bounds of EDGE_WIN;
    even traces abnormal (7000 / 1000 > 2 * 1.5), odd ones normal."""
    times = [(-10, 25, 1), (-11, 0, 0), (0, 26, 0), (-10, -10, 1), (25, 25, 1), (5, 7, 1), (-11, 26, 0),
             (-9, 24, 1), (-10, 26, 0), (-11, 25, 0)]
    tr = np.repeat(np.arange(len(times)), 2)
    op = np.tile([0, 1], len(times))
    dur = np.where(tr % 2 == 0, 7000, 2000) - np.tile([0, 1], len(times))
    ts = np.array([times[t][0] for t in tr])
    te = np.array([times[t][1] for t in tr])
    table = make_table(tr, op, dur, ts, te, n_svcops=2)
    return table, np.array([1.5, 1.5]), np.ones(2, np.uint8), np.array([t[2] for t in times], bool)


@functools.lru_cache(maxsize=None)
def edge_per_span():
    """(table, a3, ok, expected state in EDGE_WIN, rows in EDGE_WIN): per-span times.
    trace 0: its largest duration (9000) and two of its four op-0 rows lie outside; inside max 2500 against
      expect 2 * 1.0 + 1 * 0.25 = 2.25: abnormal, while the whole trace (9.0 against 4.25) and the inside max
      against the whole trace's counts (2.5 against 4.25) are not both so;
    trace 1: the same rows with the inside max 2250: a tie, normal;
    trace 2: its only positive duration lies outside: dropped, its inside rows count;
    trace 3: no row inside;
    trace 4: every row inside, rows exactly on both bounds."""
    t0, t1 = EDGE_WIN
    rows = []   # (trace, op, duration, ts, te)
    for t, mx in ((0, 2500), (1, 2250)):
        rows += [(t, 0, mx, t0, t1), (t, 0, 10, 0, 5), (t, 1, 20, 3, t1), (t, 0, 9000, t0 - 1, 5), (t, 0, 30, 0, t1 + 1)]
    rows += [(2, 0, 0, 0, 1), (2, 1, -4, 2, 3), (2, 0, 5000, t0 - 1, t1)]
    rows += [(3, 0, 800, t1, t1 + 1), (3, 1, 900, t0 - 5, t0 - 1)]
    rows += [(4, 0, 100, t0, t0), (4, 1, 200, t1, t1), (4, 1, 300, t0, t1)]
    a = np.array(rows, np.int64)
    a = a[np.random.default_rng(3).permutation(len(rows))]
    table = make_table(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], n_svcops=2)
    return table, np.array([1.0, 0.25]), np.ones(2, np.uint8), np.array([2, 1, 0, 0, 1], np.uint8), 3 + 3 + 2 + 0 + 3


@functools.lru_cache(maxsize=None)
def edge_single():
    """(table, a3, ok): one trace, one service-op, three rows; 3 * 0.5 against 1.501: abnormal."""
    table = make_table([0, 0, 0], [0, 0, 0], [1501, -2, 7], [4, 4, 4], [9, 9, 9], n_svcops=1)
    return table, np.array([0.5]), np.ones(1, np.uint8)


# ---------------------------------------------------------------------------------- D: detect_block staging
# name: (traces, (trace, service-op) entries of the first block of 256 traces, a trace of 4,100 service-ops)
STAGE_TABLES = {"nt1": (1, 4100, True), "nt255": (255, 4095, False), "nt256": (256, 4096, False),
                "nt257": (257, 4097, False), "nt513": (513, 8193, True)}
STAGE_COMMON_OPS = 1000   # tables without the 4,100-op trace stay within the layout-order build's service-op limit


def _spread(rng, n, total, lo=1):
    """n integers >= lo that add up to total."""
    assert total >= n * lo
    cut = np.sort(rng.integers(0, total - n * lo + 1, n - 1)) if n > 1 else np.zeros(0, np.int64)
    parts = np.diff(np.concatenate([[0], cut, [total - n * lo]]))
    return (parts + lo).astype(np.int64)


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """A table whose first detector block holds a chosen number of entries, a namespace (table, a3, ok,
    entries per trace, expected states).  Per trace: distinct common service-ops (a3 log-uniform in
    1e-3..1e6, about one in twelve without an SLO, 1..3 rows each) and, last in name order, one service-op
    of its own whose a3 puts the sequential expect exactly on real = max / 1000.0 (odd traces: a tie,
    normal) or one ulp below it (even traces: abnormal).  nt257: trace 255 holds entries 4090..4096 of the
    block; nt513: traces 256..511 hold one entry each, trace 3 holds 4,100 entries from entry ~2000 on."""
    nt, first, big = STAGE_TABLES[name]
    rng = np.random.default_rng(900 + nt)
    n_common = 4100 if big else STAGE_COMMON_OPS
    nb = min(nt, DB)
    ent = np.ones(nt, np.int64)
    if name == "nt1":
        ent[0] = first
    elif name == "nt513":
        ent[:3] = _spread(rng, 3, 2000, 2)
        ent[3] = 4100
        ent[4:nb] = _spread(rng, nb - 4, first - 2000 - 4100, 2)
        ent[512] = 37
    elif name == "nt257":
        ent[:255] = _spread(rng, 255, 4090, 2)
        ent[255] = 7
    else:
        ent[:nb] = _spread(rng, nb, first, 2)
    assert int(ent[:nb].sum()) == first
    a3c = 10.0 ** rng.uniform(-3, 6, n_common)
    okc = (rng.random(n_common) > 1 / 12).astype(np.uint8)
    a3 = np.concatenate([a3c, np.zeros(nt)])
    ok = np.concatenate([okc, np.ones(nt, np.uint8)])
    tr, op, du = [], [], []
    for t in range(nt):
        k = int(ent[t]) - 1
        assert k <= n_common   # common ops; the trace's own op (code n_common + t) comes last in name order
        ops = np.sort(rng.choice(n_common, k, replace=False)) if k else np.zeros(0, np.int64)
        cn = rng.integers(1, 4, k) if k else np.zeros(0, np.int64)
        part = 0.0
        for o, c in zip(ops.tolist(), cn.tolist()):
            if okc[o]:
                part = part + float(c) * float(a3c[o])
        c_own = 1
        mx = _mx_for(part * 1.0001 + 0.004)
        real = mx / 1000.0
        want = real if t % 2 else math.nextafter(real, -math.inf)
        a_own = want - part   # then nudged until fl(part + fl(1 * a_own)) is the wanted double
        for _ in range(200):
            got = part + float(c_own) * a_own
            if got == want:
                break
            a_own = math.nextafter(a_own, math.inf if got < want else -math.inf)
        assert part + a_own == want, (name, t)
        a3[n_common + t] = a_own
        codes = np.concatenate([np.repeat(ops, cn), [n_common + t]]).astype(np.int64)
        d = rng.integers(-5, 3, codes.size)
        d = np.minimum(d, mx)
        d[rng.integers(0, codes.size)] = mx
        p = rng.permutation(codes.size)
        tr.append(np.full(codes.size, t))
        op.append(codes[p])
        du.append(d[p])
    tr, op, du = np.concatenate(tr), np.concatenate(op), np.concatenate(du)
    ts = 5 * tr.astype(np.int64) - 300
    table = make_table(tr, op, du, ts, ts + 4, podop=op % 11, n_traces=nt, n_svcops=n_common + nt)
    state = np.where(np.arange(nt) % 2 == 1, 1, 2).astype(np.uint8)
    return types.SimpleNamespace(table=table, a3=a3, ok=ok, entries=ent + 0, state=state)


# ---------------------------------------------------------------------------------- E: sweep arithmetic
# (t_begin, grain, window, n_win)
SWEEPS = ((0, 7, 20, 4096), (0, 7, 20, 4097), (0, 7, 20, 1), (0, 7, 20, 0), (0, 7, 0, 4096), (0, 7, 0, 4097),
          (-50, 7, 20, 300), (1001, 3, 20, 50), (-150, 10, 20, 100), (15000, 7, 0, 9))
SWEEP_SPAN = 4097 * 7


@functools.lru_cache(maxsize=None)
def sweep_table():
    """(table, a3, ok): 200 traces of 1..5 rows with trace-level times over -300 .. 4097 * 7 + 500: lengths
    of 0 (thirty of them on multiples of 7, for window = 0), below the window of 20 and above it; every
    third trace abnormal, every seventh dropped."""
    rng = np.random.default_rng(77)
    nt = 200
    ts = rng.integers(-300, SWEEP_SPAN + 500, nt)
    ln = rng.choice([0, 0, 1, 6, 13, 19, 20, 21, 60, 400], nt)
    ts[:30] = 7 * rng.integers(-5, 4100, 30)
    ln[:30] = 0
    ts[30:34], ln[30:34] = [-3, -7, 0, 0], [5, 20, 21, 20]           # around t_begin = 0
    ts[34:38], ln[34:38] = [SWEEP_SPAN - 7, SWEEP_SPAN - 14, SWEEP_SPAN, 4095 * 7], [0, 20, 0, 20]
    ts[38:44], ln[38:44] = [-290, -200, -120, -60, SWEEP_SPAN + 100, SWEEP_SPAN + 450], [10, 0, 30, 19, 6, 0]
    sizes = rng.integers(1, 6, nt)
    tr = np.repeat(np.arange(nt), sizes)
    tr = tr[rng.permutation(tr.size)]                                 # traces interleaved
    op = rng.integers(0, 4, tr.size)
    dur = rng.integers(1, 900, tr.size)
    for t in range(nt):
        r = np.flatnonzero(tr == t)
        if t % 7 == 0:
            dur[r] = -dur[r]
        elif t % 3 == 0:
            dur[r[0]] = 50_000
    table = make_table(tr, op, dur, ts[tr], (ts + ln)[tr], n_traces=nt, n_svcops=4)
    return table, np.array([1.0, 2.0, 0.5, 4.0]), np.array([1, 1, 1, 0], np.uint8)


BIG_SWEEPS = ((-20, 10, 15, 8), (0, 5, 9, 3), (0, 20, 19, 2))


@functools.lru_cache(maxsize=None)
def sweep_big_table():
    """(table, a3, ok): one trace of 65,536 rows, one of 65,537 (the two sides of k_ix_sweep's switch to
    64-bit row counters) and one of 3, rows interleaved; times 0..9, 10..19 and 0..19."""
    sizes = np.array([65_536, 65_537, 3])
    tr = np.repeat(np.arange(3), sizes)
    tr = tr[np.random.default_rng(8).permutation(tr.size)]
    op = (np.arange(tr.size) % 2)
    dur = np.where(tr == 2, 2, 5)                 # 0.002 against 0.003: normal
    for t in (0, 1):                              # 65.537 against about 65.536 (abnormal) and about 65.537
        dur[np.flatnonzero(tr == t)[0]] = 65_537
    ts = np.array([0, 10, 0])[tr]
    te = np.array([9, 19, 19])[tr]
    table = make_table(tr, op, dur, ts, te, n_traces=3, n_svcops=2)
    return table, np.array([0.001, 0.001]), np.ones(2, np.uint8)


# ---------------------------------------------------------------------------------- GPU callers
def detect_call(ctx, dev, t0, t1, a3, ok):
    """(status, state, n_abnormal, n_normal, n_spans_in_window) of one mr_detect call; state pre-filled 9."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    a3, ok = np.ascontiguousarray(a3, np.float64), np.ascontiguousarray(ok, np.uint8)
    state = np.full(dev.table.n_traces, 9, np.uint8)
    na, nn, nin = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    rc = _lib.load().mr_detect(ctx.h, dev.h, t0, t1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), ptr(state, C.c_uint8),
                               C.byref(na), C.byref(nn), C.byref(nin))
    return rc, state, na.value, nn.value, nin.value


def check_detect(ctx, dev, table, t0, t1, a3, ok):
    """One mr_detect call against the oracle, exactly; returns the expected state (None: an empty window)."""
    from microrank_amd import _lib

    state, na, nn, rows = detect_oracle(table, t0, t1, a3, ok)
    rc, gs, gna, gnn, gin = detect_call(ctx, dev, t0, t1, a3, ok)
    if state is None:
        assert rc == _lib.MR_ERR_VALUE and gin == 0
        return None
    assert rc == _lib.MR_OK
    assert (gna, gnn, gin) == (na, nn, rows)
    assert gs.tolist() == state.tolist()
    return state


def sweep_call(ctx, dev, t_begin, grain, window, n_win, a3, ok):
    """(status, state, n_abnormal, n_normal, n_rows) of one mr_detect_sweep call, outputs pre-filled."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    a3, ok = np.ascontiguousarray(a3, np.float64), np.ascontiguousarray(ok, np.uint8)
    state = np.full(dev.table.n_traces, 9, np.uint8)
    na, nn = np.full(max(n_win, 1), -7, np.int32), np.full(max(n_win, 1), -7, np.int32)
    rows = np.full(max(n_win, 1), -7, np.int64)
    rc = _lib.load().mr_detect_sweep(ctx.h, dev.h, t_begin, grain, window, n_win, ptr(a3, C.c_double), ptr(ok, C.c_uint8),
                                     ptr(state, C.c_uint8), ptr(na, C.c_int32), ptr(nn, C.c_int32), ptr(rows, C.c_int64))
    return rc, state, na[:n_win], nn[:n_win], rows[:n_win]


def check_sweep(ctx, dev, table, t_begin, grain, window, n_win, a3, ok):
    from microrank_amd import _lib

    state, na, nn, rows = sweep_oracle(table, a3, ok, t_begin, grain, window, n_win)
    rc, gs, gna, gnn, grows = sweep_call(ctx, dev, t_begin, grain, window, n_win, a3, ok)
    assert rc == _lib.MR_OK
    assert grows.dtype == np.int64 and grows.tolist() == rows.tolist()
    assert gna.tolist() == na.tolist() and gnn.tolist() == nn.tolist()
    assert gs.tolist() == state.tolist()
    return na, nn, rows


def rca_call(ctx, dev, t0, t1, a3, ok, top_max=5):
    """(status, codes, scores, n_abnormal, n_normal) of one mr_rca_window call (fp64, dstar2)."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    a3, ok = np.ascontiguousarray(a3, np.float64), np.ascontiguousarray(ok, np.uint8)
    codes, scores = np.zeros(top_max + 6, np.int32), np.zeros(top_max + 6)
    n_out, na, nn, edges = C.c_int32(), C.c_int32(-7), C.c_int32(-7), C.c_int64()
    rc = _lib.load().mr_rca_window(ctx.h, dev.h, t0, t1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), 0, top_max, _lib.MR_FP64,
                                   ptr(codes, C.c_int32), ptr(scores, C.c_double), C.byref(n_out), C.byref(edges),
                                   C.byref(na), C.byref(nn))
    return rc, codes[:n_out.value].copy(), scores[:n_out.value].copy(), na.value, nn.value


def fused_counts(ctx, dev, windows, a3, ok):
    """[(status, n_abnormal, n_normal)] per window from ONE mr_windows_batch call, and per window from its
    own mr_rca_window call: the detectors fused into the window builds.  Both must agree."""
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows

    got = rank_windows(ctx, [(dev, t0, t1, a3, ok) for t0, t1 in windows])
    out = []
    for (t0, t1), (_, _, na, nn, _, status) in zip(windows, got):
        rc, _, _, na1, nn1 = rca_call(ctx, dev, t0, t1, a3, ok)
        assert rc == status
        if rc == _lib.MR_OK:
            assert (int(na), int(nn)) == (na1, nn1)
        out.append((int(status), int(na), int(nn)))
    return out


def check_fused_counts(ctx, dev, table, windows, a3, ok):
    """mr_windows_batch's and mr_rca_window's detector counts of every window against the oracle."""
    from microrank_amd import _lib

    for (t0, t1), (status, na, nn) in zip(windows, fused_counts(ctx, dev, windows, a3, ok)):
        state, ena, enn, _ = detect_oracle(table, t0, t1, a3, ok)
        if state is None:
            assert status == _lib.MR_ERR_VALUE, (t0, t1)
        else:
            assert (status, na, nn) == (_lib.MR_OK, ena, enn), (t0, t1)


def export_graph(ctx, table, dev, sel):
    """(PagerankGraph, its mr_graph_export arrays) of mr_graph_build over the traces of `sel`."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.preprocess_data import PagerankGraph

    pg = PagerankGraph(ctx, table, dev, np.asarray(sel).astype(np.uint8))
    dg = pg.device_graph()
    info = dg.info()
    N, T, nnz, E = info["N"], info["T"], info["nnz"], info["E"]
    ex = dict(sr_off=np.empty(T + 1, np.int64), sr_ops=np.empty(nnz, np.int32), len_t=np.empty(T, np.int32),
              len_o=np.empty(N, np.int32), ss_off=np.empty(N + 1, np.int64), ss_par=np.empty(E, np.int32),
              nchild=np.empty(N, np.int32))
    ctx.check(_lib.load().mr_graph_export(dg.h, ptr(ex["sr_off"], C.c_int64), ptr(ex["sr_ops"], C.c_int32),
                                          ptr(ex["len_t"], C.c_int32), ptr(ex["len_o"], C.c_int32),
                                          ptr(ex["ss_off"], C.c_int64), ptr(ex["ss_par"], C.c_int32),
                                          ptr(ex["nchild"], C.c_int32)), "mr_graph_export")
    return pg, ex


def check_graph(ctx, table, dev, sel, cols=None):
    """mr_graph_build + mr_graph_export over `sel` against oracle.span_graph on the same rows, exactly;
    len_t also against the plain per-trace row count.  cols: the table's code columns when the table does
    not hold them as arrays.  Returns len_t."""
    import oracle as orc

    trace, podop, span, parent = cols if cols is not None else (table.trace, table.podop, table.span, table.parent)
    sel = np.asarray(sel, bool)
    pg, ex = export_graph(ctx, table, dev, sel)
    sg = orc.span_graph(trace, podop, span, parent, sel)
    assert pg.trace_code.tolist() == sg.trace_codes.tolist()
    n_rows = np.bincount(trace, minlength=sel.size)
    assert ex["len_t"].tolist() == n_rows[pg.trace_code].tolist()
    assert ex["len_t"].tolist() == sg.len_t.tolist()
    assert pg.node_podop.tolist() == sg.node_podop.tolist()
    assert ex["len_o"].tolist() == sg.len_o.tolist()
    assert ex["nchild"].tolist() == sg.nchild.tolist()
    assert np.repeat(np.arange(sg.trace_codes.size), np.diff(ex["sr_off"])).tolist() == sg.sr_t.tolist()
    assert ex["sr_ops"].tolist() == sg.sr_o.tolist()
    assert np.repeat(np.arange(sg.node_podop.size), np.diff(ex["ss_off"])).tolist() == sg.ss_c.tolist()
    assert ex["ss_par"].tolist() == sg.ss_p.tolist()
    return ex["len_t"]
