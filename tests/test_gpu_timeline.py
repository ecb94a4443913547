"""GPU checks of mr_windows_timeline (csrc/mr_timeline.hip): per asked pod-op -- and for the window's own
traces -- the count, the summed and the largest value per time bucket on each side of the window's detector
partition.  Every comparison is exact integer equality of all four outputs with the numpy oracle of
tests/timeline_cases.py (the span table's rows and oracle.detect's partition); no tolerance anywhere."""
import contextlib
import csv
import ctypes as C
import io
import os

import numpy as np
import pandas as pd
import pytest

import call_edge_cases as ce
import kind_breakdown_cases as kb
import latency_cases as lc
import timeline_cases as tc
from timeline_cases import K_TOP, NAMES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def five():
    """The five oracle windows on the device: (ctx, [window cases], [(DeviceSpans, t0, t1, a3, ok)])."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    cases = [tc.window(n) for n in NAMES]
    devs = [DeviceSpans(ctx, w.table) for w in cases]
    yield ctx, cases, [(d, w.t0, w.t1, w.a3, w.ok) for d, w in zip(devs, cases)]
    for d in devs:
        d.close()


def _grids(cases, B, kind):
    g = [tc.grid(w, B, kind) for w in cases]
    return [x[0] for x in g], [x[1] for x in g]


@pytest.mark.parametrize("kind", ["default", "off"])
@pytest.mark.parametrize("what", tc.WHATS)
@pytest.mark.parametrize("B", tc.BUCKETS)
def test_oracle_equality_in_one_call_and_alone(five, B, what, kind):
    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    b0, bw = _grids(cases, B, kind)
    _, out, status = tc.call(ctx, wins, ops, K_TOP, B, what, b0, bw)
    assert status.tolist() == [0] * len(wins)
    for w, o in zip(cases, out):
        tc.same(o, tc.expected(w.name, B, what, kind))
    for i, w in enumerate(cases):
        _, alone, st = tc.call(ctx, wins[i:i + 1], ops[i:i + 1], K_TOP, B, what, b0[i:i + 1], bw[i:i + 1])
        assert st.tolist() == [0] and tc.raw_bytes(alone) == tc.raw_bytes(out[i:i + 1]), w.name


@pytest.mark.parametrize("blocks", [None, "1", "7"])
def test_boundary_table(blocks, monkeypatch):
    """Every grid of the boundary table, both values; `main` and `wide4` (four buckets each) in ONE call too:
    a call's windows bring their own origin and width."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    b = tc.boundary()
    asked = tc.boundary_ops()
    if blocks is not None:
        monkeypatch.setenv("MR_TL_BLOCKS", blocks)
    ctx = _lib.default_context()
    dev = DeviceSpans(ctx, b.table)
    try:
        win = (dev, b.t0, b.t1, b.a3, b.ok)
        for what in tc.WHATS:
            for name, (b0, bw, B) in tc.GRIDS.items():
                _, out, st = tc.call(ctx, [win], [asked], len(asked), B, what, [b0], [bw])
                assert st.tolist() == [0]
                tc.same(out[0], tc.boundary_expected(name, what))
            two = [tc.GRIDS["main"], tc.GRIDS["wide4"]]
            _, out, st = tc.call(ctx, [win, win], [asked, asked], len(asked), 4, what, [g[0] for g in two], [g[1] for g in two])
            assert st.tolist() == [0, 0]
            tc.same(out[0], tc.boundary_expected("main", what))
            tc.same(out[1], tc.boundary_expected("wide4", what))
    finally:
        dev.close()


def test_invariance_under_blocks_chunks_and_order(five, monkeypatch):
    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    for B in (30, 512):   # (the direct-mapped and the hashed table of a block)
        b0, bw = _grids(cases, B, "off")
        _, out, status = tc.call(ctx, wins, ops, K_TOP, B, "self", b0, bw)
        ref = tc.raw_bytes(out)
        for name, values in (("MR_TL_BLOCKS", ("1", "7")), ("MR_TL_CHUNK", ("1", "2"))):   # (both read per call)
            for v in values:
                monkeypatch.setenv(name, v)
                _, o, s = tc.call(ctx, wins, ops, K_TOP, B, "self", b0, bw)
                assert tc.raw_bytes(o) == ref and s.tolist() == status.tolist(), (name, v)
            monkeypatch.delenv(name)
        _, o, s = tc.call(ctx, wins[::-1], ops[::-1], K_TOP, B, "self", b0[::-1], bw[::-1])
        assert tc.raw_bytes(o[::-1]) == ref and s[::-1].tolist() == status.tolist()
        _, o, s = tc.call(ctx, wins, ops, K_TOP, B, "self", b0, bw)   # and twice the same
        assert tc.raw_bytes(o) == ref


def _windows_latency(ctx, wins, ops, what, q, method):
    """mr_windows_latency over the op slots of ops (-1 left out): (out[n, K, 2, 1], count[n, K, 2])."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    n = len(wins)
    spans = (_lib.P * n)(*[w[0].h for w in wins])
    t0, t1 = np.array([w[1] for w in wins], np.int64), np.array([w[2] for w in wins], np.int64)
    a3 = (C.c_void_p * n)(*[w[3].ctypes.data for w in wins])
    ok = (C.c_void_p * n)(*[w[4].ctypes.data for w in wins])
    cod = np.zeros((n, K_TOP), np.int32)
    n_ops = np.array([len(o) for o in ops], np.int32)
    for i, o in enumerate(ops):
        cod[i, :len(o)] = o
    qv = np.array([q], np.float64)
    out, cnt, status = np.zeros((n, K_TOP, 2, 1)), np.zeros((n, K_TOP, 2), np.int64), np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_latency(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                             ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), K_TOP, lc.WHAT[what],
                                             ptr(qv, C.c_double), 1, lc.METHODS[method], ptr(out, C.c_double),
                                             ptr(cnt, C.c_int64), ptr(status, C.c_int32)), "mr_windows_latency")
    return out, cnt


def test_cross_checks_against_the_shipped_entries(five):
    """Per op and side, buckets + out == mr_windows_latency's count; with one bucket over everything tl_max ==
    its q = 1 `higher` quantile (exact: every value of these windows is far below 2^53); slot -1's totals ==
    mr_windows_kind_breakdown's kb_tot of -1 (abnormal, normal)."""
    ctx, cases, wins = five
    asked = [tc.asked_ops(w) for w in cases]
    only = [[c for c in a if c >= 0] for a in asked]
    b0, bw = _grids(cases, 30, "off")
    assert all(0 <= w.table.tstart.min() and w.table.tstart.max() < tc.BIG for w in cases)
    checked = 0
    for what in tc.WHATS:
        q1, count = _windows_latency(ctx, wins, only, what, 1.0, "higher")
        _, out, _ = tc.call(ctx, wins, only, K_TOP, 30, what, b0, bw)
        # B = 1 over [0, 2^62): one bucket that holds every start of these tables
        _, one, _ = tc.call(ctx, wins, only, K_TOP, 1, what, [0] * len(cases), [tc.BIG] * len(cases))
        for i, w in enumerate(cases):
            assert (out[i].cnt.sum(axis=1) + out[i].out.sum(axis=2)).tolist() == count[i].tolist(), (w.name, what)
            assert one[i].cnt[:, 0].tolist() == count[i].tolist() and not one[i].out.any()
            assert np.abs(lc.values(w.table, what)).max() < 1 << 53
            assert one[i].max[:, 0].astype(np.float64).tolist() == q1[i, :, :, 0].tolist(), (w.name, what)
            checked += int((count[i] > 0).sum())
    assert checked > 50
    _, kout, _ = kb.call(ctx, wins, [[-1]] * len(cases), 1, 1)
    _, out, _ = tc.call(ctx, wins, [[-1]] * len(cases), 1, 30, "self", b0, bw)
    for i, w in enumerate(cases):
        tot = out[i].cnt[0].sum(axis=0) + out[i].out[0].sum(axis=1)   # [normal, abnormal]
        assert [int(tot[1]), int(tot[0])] == kout[i].tot[0].tolist() == [int((w.state == 2).sum()), int((w.state == 1).sum())]


def test_empty_window_beside_a_good_one(five):
    from microrank_amd import _lib

    ctx, cases, wins = five
    ops = tc.asked_ops(cases[0])
    b0, bw = tc.grid(cases[0], 30)
    empty = (wins[0][0], 0, 1, wins[0][3], wins[0][4])   # no trace in [0, 1] ns
    _, out, status = tc.call(ctx, [empty, wins[0]], [ops, ops], K_TOP, 30, "self", [0, b0], [1, bw])
    assert status.tolist() == [_lib.MR_ERR_VALUE, 0]
    tc.same(out[0], tc.timeline_oracle(cases[0].table, None, ops, K_TOP, 30, "self", 0, 1))
    tc.same(out[1], tc.expected(cases[0].name, 30, "self"))


def test_whole_table_window(five):
    """INT64_MIN / INT64_MAX: the whole table, as in mr_op_latency; the grid is the caller's."""
    ctx, cases, wins = five
    w, win = cases[2], wins[2]
    ops = tc.asked_ops(w)
    b0, bw = tc.grid(w, 7, "off")
    _, out, status = tc.call(ctx, [(win[0], tc.I64_MIN, tc.I64_MAX, win[3], win[4])], [ops], K_TOP, 7, "self", [b0], [bw])
    assert status.tolist() == [0]
    tc.same(out[0], tc.expected(w.name, 7, "self", "off"))   # (the named windows span their tables)


def test_errors_leave_the_context_usable(five):
    import dataclasses

    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    b0, bw = _grids(cases, 7, "default")

    def good():
        _, out, status = tc.call(ctx, wins[:1], ops[:1], K_TOP, 7, "self", b0[:1], bw[:1])
        assert status.tolist() == [0]
        tc.same(out[0], tc.expected(cases[0].name, 7, "self"))

    bad_calls = [
        dict(k=0), dict(k=65), dict(B=0), dict(B=513), dict(what=2), dict(what=-1),
        dict(bw=[0] + bw[1:]), dict(bw=[-5] + bw[1:]),
        dict(ops=[list(range(12))] + ops[1:]),                      # n_ops[i] outside 0..K
        dict(ops=[[0, cases[0].table.n_podops]] + ops[1:]),         # a code outside [-1, n_podops)
        dict(ops=[[0, -2]] + ops[1:]),
    ]
    for bad in bad_calls:
        kw = dict(wins=wins, ops=ops, k=K_TOP, B=7, what="self", bw=bw)
        kw.update(bad)
        rc, _, _ = tc.call(ctx, kw["wins"], kw["ops"], kw["k"], kw["B"], kw["what"], b0, kw["bw"], check=False)
        assert rc == _lib.MR_ERR_ARG, bad
        good()
    rc, _, _ = tc.call(ctx, wins, ops, K_TOP, 7, "self", b0, bw, check=False, n_ops=[-1] + [len(o) for o in ops[1:]])
    assert rc == _lib.MR_ERR_ARG
    good()
    # a null pointer
    n1 = np.zeros(1, np.int32)
    rc = _lib.load().mr_windows_timeline(ctx.h, 1, None, None, None, None, None, None, _lib.ptr(n1, C.c_int32), 1, 0, None,
                                         None, 1, None, None, None, None, None)
    assert rc == _lib.MR_ERR_ARG
    good()
    other = _lib.Context()   # a table of another context
    try:
        odev = DeviceSpans(other, cases[0].table)
        rc, _, _ = tc.call(ctx, [(odev,) + wins[0][1:]], ops[:1], K_TOP, 7, "self", b0[:1], bw[:1], check=False)
        assert rc == _lib.MR_ERR_ARG
        odev.close()
    finally:
        other.close()
    good()
    # MR_ERR_STATE, in the header's order; the message names the case.  A table without time columns (the
    # whole-table window included, and before anything else is looked at: it is asked -1 with self time); a
    # table of per-span window times (the whole-table window included); self time on a trace shard (-1 asked
    # too: the self time is named); -1 on a trace shard; -1 on a table without the per-trace index (an empty
    # table is never indexed).
    timeless = lc.banded_table(times=False)[0]
    st = ce.window("span_times").table
    full = cases[0].table
    shard = full.shard(0, 2)
    assert shard.row is not None and 0 < shard.n_spans < full.n_spans
    none = full.take(np.zeros(0, np.int64))
    assert none.n_spans == 0 and none.n_podops == full.n_podops
    timeless_shard = dataclasses.replace(shard, tstart=None, tend=None)
    whole = (tc.I64_MIN, tc.I64_MAX)
    for table, win, asked, what, word in ((timeless, whole, [0, -1], "self", "startTime/endTime"),
                                          (timeless, (0, 1), [0], "duration", "startTime/endTime"),
                                          (timeless_shard, whole, [0, -1], "self", "startTime/endTime"),
                                          (st, None, [0], "duration", "trace-level times"),
                                          (st, whole, [0, -1], "self", "trace-level times"),
                                          (shard, None, [0, -1], "self", "self time on a trace shard"),
                                          (shard, None, [0, -1], "duration", "slot -1 on a trace shard"),
                                          (none, (0, 1), [-1], "duration", "per-trace index"),
                                          (none, whole, [0, -1], "self", "per-trace index")):
        dev = DeviceSpans(ctx, table)
        try:
            a3, ok = np.full(table.n_svcops, 1.0), np.ones(table.n_svcops, np.uint8)
            w0, w1 = win if win is not None else (int(table.tstart.min()), int(table.tend.max()))
            rc, _, _ = tc.call(ctx, [(dev, w0, w1, a3, ok)], [asked], 2, 4, what, [0], [1000], check=False)
            assert rc == _lib.MR_ERR_STATE, word
            assert word in _lib.load().mr_last_error(ctx.h).decode(), word
        finally:
            dev.close()
        good()


def test_op_slots_on_a_trace_shard(five):
    """Op slots with MR_LAT_DURATION on a trace shard are allowed: they cover that rank's rows under that rank's
    detector partition -- the oracle on the shard's own table."""
    import oracle as orc
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, _ = five
    w = cases[0]
    shard = w.table.shard(1, 2)
    res = orc.detect(shard.trace, shard.svcop, shard.duration, shard.tstart, shard.tend, w.t0, w.t1,
                     {i: float(w.a3[i]) for i in range(w.a3.size) if w.ok[i]})
    state = kb.state_of(shard.n_traces, res[1], res[2])
    asked = [c for c in tc.asked_ops(w) if c >= 0]
    b0, bw = tc.grid(w, 30)
    dev = DeviceSpans(ctx, shard)
    try:
        _, out, status = tc.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [asked], K_TOP, 30, "duration", [b0], [bw])
    finally:
        dev.close()
    assert status.tolist() == [0]
    exp = tc.timeline_oracle(shard, state, asked, K_TOP, 30, "duration", b0, bw, w.t0, w.t1)
    tc.same(out[0], exp)
    assert 0 < exp.cnt.sum() < tc.expected(w.name, 30, "duration").cnt.sum()


# ---------------------------------------------------------------------------------- the Python surface
def _as_lists(e, j):
    return {"cnt": e.cnt[j].tolist(), "sum": e.sum[j].tolist(), "max": e.max[j].tolist(), "out": e.out[j].tolist()}


def test_windows_timeline_python(five):
    from microrank_amd.online_rca import windows_timeline

    ctx, cases, wins = five
    asked = [tc.asked_ops(w) for w in cases]
    got = windows_timeline(ctx, wins, asked, buckets=30, what="duration")
    assert len(got) == len(cases)
    for w, a, g in zip(cases, asked, got):
        e = tc.expected(w.name, 30, "duration")
        b0, bw = tc.grid(w, 30)
        assert list(g) == list(dict.fromkeys(a))
        for j, c in enumerate(a):
            assert {k: v.tolist() for k, v in g[c].items() if k != "start"} == _as_lists(e, j)
            assert g[c]["start"].tolist() == [b0 + b * bw for b in range(30)] and not g[c]["out"].any()
    # the caller's grid: one origin / width per window
    b0, bw = _grids(cases, 7, "off")
    got = windows_timeline(ctx, wins, asked, buckets=7, origin=b0, width=bw)
    for w, a, g in zip(cases, asked, got):
        e = tc.expected(w.name, 7, "self", "off")
        assert all({k: v.tolist() for k, v in g[c].items() if k != "start"} == _as_lists(e, j) for j, c in enumerate(a))
    assert windows_timeline(ctx, [], []) == []


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden, regen_window

    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


def _named_oracle(adf, slo, operation_list, start, end, ops, B):
    """{-1 / op name: window_timeline's lists} by names from the DataFrame's own factorisation and the reference
    detector's lists, over the default grid."""
    from microrank_amd.anormaly_detector import system_anomaly_detect
    from microrank_amd.spans import SpanTable

    with contextlib.redirect_stdout(io.StringIO()):
        flag, abnormal, normal = system_anomaly_detect(adf, start_time=start, end_time=end, slo=slo,
                                                       operation_list=operation_list)
    assert flag is True and abnormal and normal
    table = SpanTable.from_dataframe(adf)
    code = {n: i for i, n in enumerate(table.trace_names)}
    state = kb.state_of(table.n_traces, [code[t] for t in abnormal], [code[t] for t in normal])
    pcode = {n: i for i, n in enumerate(table.podop_names)}
    asked = [-1] + [pcode[o] for o in ops]
    t0, t1 = int(pd.Timestamp(start).value), int(pd.Timestamp(end).value)
    b0, bw = t0, (t1 - t0) // B + 1
    e = tc.timeline_oracle(table, state, asked, len(asked), B, "self", b0, bw, t0, t1)
    return {key: dict(_as_lists(e, j), start=[b0 + b * bw for b in range(B)]) for j, key in enumerate([-1] + list(ops))}


def test_rca_window_timeline(golden):
    from microrank_amd.online_rca import rca_window, window_timeline

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo)
    assert plain["top"]
    with_tl = rca_window(adf, start, end, slo, timeline=6)
    tl = with_tl.pop("timeline")
    assert with_tl == plain                          # every other key is what it was
    assert tl == window_timeline(adf, start, end, slo, plain["top"], buckets=6)
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 6)
    assert list(tl) == list(exp) and tl == exp
    assert sum(sum(x) for x in tl[-1]["cnt"]) == plain["n_abnormal"] + plain["n_normal"] and tl[-1]["out"] == [[0, 0], [0, 0]]


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


def test_driver_writes_timeline_csv(golden, tmp_path, monkeypatch):
    c, adf, slo = golden
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_plain = _drive(adf, slo, c["operation_list"])
    assert os.path.exists("result.csv") and not os.path.exists("timeline.csv")   # without the keyword: no file
    monkeypatch.chdir(tmp_path / "b")
    out_tl = _drive(adf, slo, c["operation_list"], timeline=6)
    assert out_tl == out_plain
    assert open("result.csv", "rb").read() == open(tmp_path / "a" / "result.csv", "rb").read()
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    rows = list(csv.reader(open("timeline.csv")))
    assert rows[0] == ["result", "rank", "bucket", "start", "count_abnormal", "count_normal", "mean_abnormal", "mean_normal",
                       "max_abnormal", "max_normal"]
    # the data holds one 5-minute window of traffic: the one trigger is the driver's first window
    start = adf["startTime"].min()
    exp = _named_oracle(adf, slo, c["operation_list"], start, start + pd.Timedelta(minutes=5), ranked, 6)
    want = [(label, str(rank), str(b), str(e["start"][b]), e["cnt"][b][1], e["cnt"][b][0], e["sum"][b][1], e["sum"][b][0],
             e["max"][b][1], e["max"][b][0])
            for rank, (label, e) in enumerate([("*", exp[-1])] + [(r, exp[r]) for r in ranked]) for b in range(6)]
    assert len(rows) - 1 == 6 * (1 + len(ranked)) and len(ranked) > 2
    assert [tuple(x[:6]) for x in rows[1:]] == [w[:4] + (str(w[4]), str(w[5])) for w in want]
    # the value columns, not by the writer's own expression: a value of the file is in ms with four decimals, so
    # value * 1000 is within 0.05 units (half a step of 0.1) of the exact quotient of the oracle's integers,
    # plus the float64 rounding of a value of this size
    from fractions import Fraction

    some = 0
    for x, w in zip(rows[1:], want):
        ca, cn, sa, sn, xa, xn = w[4:]
        exact = [Fraction(sa, ca) if ca else Fraction(0), Fraction(sn, cn) if cn else Fraction(0), Fraction(xa), Fraction(xn)]
        for text, q in zip(x[6:], exact):
            v = float(text)
            assert repr(v) == text and round(v, 4) == v
            assert abs(Fraction(v) * 1000 - q) <= Fraction(5, 100) + abs(q) * Fraction(1, 10**12), (x, q)
            some += q != 0
    assert some > 8
    assert sorted(os.listdir(".")) == ["result.csv", "timeline.csv"]
