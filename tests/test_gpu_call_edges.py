"""GPU checks of mr_windows_call_edges (csrc/mr_call_edges.hip): per asked pod-op its callers and callees
with their calls, summed and largest child duration on each side of the window's detector partition.
Every comparison is exact integer equality of all seven outputs with the numpy oracle of
tests/call_edge_cases.py (the span table's rows and oracle.detect's partition); no tolerance anywhere."""
import contextlib
import csv
import ctypes as C
import io
import os
import types

import numpy as np
import pandas as pd
import pytest

import call_edge_cases as ce
from call_edge_cases import K_TOP

pytestmark = pytest.mark.gpu

NAMES = ce.WINDOWS + ("fault",)


@pytest.fixture(scope="module")
def five():
    """The five oracle windows on the device: (ctx, [window cases], [(DeviceSpans, t0, t1, a3, ok)])."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    cases = [ce.window(n) for n in NAMES]
    devs = [DeviceSpans(ctx, w.table) for w in cases]
    yield ctx, cases, [(d, w.t0, w.t1, w.a3, w.ok) for d, w in zip(devs, cases)]
    for d in devs:
        d.close()


def _one(ctx, w, asked, k, m):
    """One window on a table of its own: (outputs, status)."""
    from microrank_amd.preprocess_data import DeviceSpans

    dev = DeviceSpans(ctx, w.table)
    try:
        _, out, status = ce.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [asked], k, m)
    finally:
        dev.close()
    return out[0], status[0]


@pytest.mark.parametrize("m", ce.MS)
def test_oracle_equality_in_one_call_and_alone(five, m):
    ctx, cases, wins = five
    ops = [ce.asked_ops(w) for w in cases]
    _, out, status = ce.call(ctx, wins, ops, K_TOP, m)
    assert status.tolist() == [0] * len(wins)
    for w, o in zip(cases, out):
        ce.same(o, ce.expected(w.name, m))
    for i, w in enumerate(cases):
        _, alone, st = ce.call(ctx, wins[i:i + 1], ops[i:i + 1], K_TOP, m)
        assert st.tolist() == [0] and ce.raw_bytes(alone) == ce.raw_bytes(out[i:i + 1]), w.name


@pytest.mark.parametrize("blocks", [None, "1", "7"])
def test_boundary_table(blocks, monkeypatch):
    from microrank_amd import _lib

    b = ce.boundary()
    asked = ce.boundary_ops()
    if blocks is not None:
        monkeypatch.setenv("MR_CE_BLOCKS", blocks)
    out, st = _one(_lib.default_context(), b, asked, len(asked), 32)
    assert st == 0
    ce.same(out, ce.boundary_expected())


def test_invariance_under_blocks_chunks_and_order(five, monkeypatch):
    ctx, cases, wins = five
    ops = [ce.asked_ops(w) for w in cases]
    _, out, status = ce.call(ctx, wins, ops, K_TOP, 8)
    ref = ce.raw_bytes(out)
    for name, values in (("MR_CE_BLOCKS", ("1", "7")), ("MR_CE_CHUNK", ("1", "2"))):   # (both read per call)
        for v in values:
            monkeypatch.setenv(name, v)
            _, o, s = ce.call(ctx, wins, ops, K_TOP, 8)
            assert ce.raw_bytes(o) == ref and s.tolist() == status.tolist(), (name, v)
        monkeypatch.delenv(name)
    _, o, s = ce.call(ctx, wins[::-1], ops[::-1], K_TOP, 8)
    assert ce.raw_bytes(o[::-1]) == ref and s[::-1].tolist() == status.tolist()
    _, o, s = ce.call(ctx, wins, ops, K_TOP, 8)   # and twice the same
    assert ce.raw_bytes(o) == ref


def test_callee_totals_equal_the_products_graph(five):
    """ce_tot of direction 1 for op a, side s == nchild[a] (the children-multiset size) of mr_graph_build over
    that side's traces of the same window, read with mr_graph_export."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.preprocess_data import PagerankGraph

    ctx, cases, wins = five
    checked = 0
    for w, win in zip(cases[:3], wins[:3]):
        ops = ce.asked_ops(w)
        _, out, _ = ce.call(ctx, [win], [ops], K_TOP, 1)
        for side in (0, 1):
            pg = PagerankGraph(ctx, w.table, win[0], (w.state == side + 1).astype(np.uint8))
            nchild = np.empty(pg.N, np.int32)
            ctx.check(_lib.load().mr_graph_export(pg.device_graph().h, None, None, None, None, None, None,
                                                  ptr(nchild, C.c_int32)), "mr_graph_export")
            of = {int(c): int(n) for c, n in zip(pg.node_podop, nchild)}
            for j, a in enumerate(ops):
                assert int(out[0].tot[j, 1, side]) == of.get(a, 0), (w.name, side, a)
                checked += of.get(a, 0) > 0
    assert checked > 10


def test_empty_window_beside_a_good_one(five):
    from microrank_amd import _lib

    ctx, cases, wins = five
    ops = ce.asked_ops(cases[0])
    empty = (wins[0][0], 0, 1, wins[0][3], wins[0][4])   # no trace in [0, 1] ns
    _, out, status = ce.call(ctx, [empty, wins[0]], [ops, ops], K_TOP, 8)
    assert status.tolist() == [_lib.MR_ERR_VALUE, 0]
    ce.same(out[0], ce.call_oracle(cases[0].table, None, ops, K_TOP, 8))
    ce.same(out[1], ce.expected(cases[0].name, 8))


def test_whole_table_window(five):
    """INT64_MIN / INT64_MAX: the whole table, as in mr_op_latency."""
    ctx, cases, wins = five
    w, win = cases[2], wins[2]
    ops = ce.asked_ops(w)
    _, out, status = ce.call(ctx, [(win[0], ce.I64_MIN, ce.I64_MAX, win[3], win[4])], [ops], K_TOP, 8)
    assert status.tolist() == [0]
    ce.same(out[0], ce.call_oracle(w.table, w.state, ops, K_TOP, 8))   # (the named windows span their tables)


def test_whole_table_of_per_span_times():
    """The whole table of a table whose window times vary within a trace: the row-level detector, which
    reads its sizes back per window (the one path with a host round trip before the chunk's read-back)."""
    from microrank_amd import _lib

    w = ce.window("span_times")
    per_trace = [np.unique(w.table.tstart[w.table.trace == t]).size for t in range(8)]
    assert max(per_trace) > 1                                   # times really vary within a trace
    assert (w.state == 1).any() and (w.state == 2).any()
    asked = ce.asked_ops(w)
    whole = types.SimpleNamespace(table=w.table, t0=ce.I64_MIN, t1=ce.I64_MAX, a3=w.a3, ok=w.ok)
    exp = ce.call_oracle(w.table, w.state, asked, K_TOP, 8)     # (the case's window spans its table)
    assert exp.peers.sum() > 0
    out, st = _one(_lib.default_context(), whole, asked, K_TOP, 8)
    assert st == 0
    ce.same(out, exp)
    # twice in one call, beside a trace-level-times window: a chunk with both detector paths
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    t = ce.window("ragged")
    d0, d1 = DeviceSpans(ctx, w.table), DeviceSpans(ctx, t.table)
    try:
        ops = [asked, ce.asked_ops(t), asked]
        wins = [(d0, ce.I64_MIN, ce.I64_MAX, w.a3, w.ok), (d1, t.t0, t.t1, t.a3, t.ok), (d0, ce.I64_MIN, ce.I64_MAX, w.a3, w.ok)]
        _, outs, status = ce.call(ctx, wins, ops, K_TOP, 8)
        assert status.tolist() == [0, 0, 0]
        ce.same(outs[0], exp)
        ce.same(outs[1], ce.expected("ragged", 8))
        ce.same(outs[2], exp)
    finally:
        d0.close()
        d1.close()


def test_more_than_4096_pod_ops():
    from microrank_amd import _lib

    w = ce.wide()
    asked = ce.WIDE_ASKED
    out, st = _one(_lib.default_context(), w, asked, len(asked), 8)
    assert st == 0
    ce.same(out, ce.call_oracle(w.table, w.state, asked, len(asked), 8, w.t0, w.t1))


def test_errors_leave_the_context_usable(five):
    import window_exemplar_cases as wx
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, wins = five
    ops = [ce.asked_ops(w) for w in cases]

    def good():
        _, out, status = ce.call(ctx, wins[:1], ops[:1], K_TOP, 8)
        assert status.tolist() == [0]
        ce.same(out[0], ce.expected(cases[0].name, 8))

    bad_calls = [
        dict(k=0), dict(k=65), dict(m=0), dict(m=33),
        dict(ops=[list(range(12))] + ops[1:]),                      # n_ops[i] outside 0..K
        dict(ops=[[0, cases[0].table.n_podops]] + ops[1:]),         # a code outside [0, n_podops)
        dict(ops=[[0, -1]] + ops[1:]),
    ]
    for bad in bad_calls:
        kw = dict(wins=wins, ops=ops, k=K_TOP, m=8)
        kw.update(bad)
        rc, _, _ = ce.call(ctx, kw["wins"], kw["ops"], kw["k"], kw["m"], check=False)
        assert rc == _lib.MR_ERR_ARG, bad
        good()
    rc, _, _ = ce.call(ctx, wins, ops, K_TOP, 8, check=False, n_ops=[-1] + [len(o) for o in ops[1:]])   # n_ops[i] < 0
    assert rc == _lib.MR_ERR_ARG
    good()
    # a null pointer
    n1 = np.zeros(1, np.int32)
    rc = _lib.load().mr_windows_call_edges(ctx.h, 1, None, None, None, None, None, None, _lib.ptr(n1, C.c_int32), 1, 1,
                                           None, None, None, None, None, None, None, None)
    assert rc == _lib.MR_ERR_ARG
    good()
    other = _lib.Context()   # a table of another context
    try:
        odev = DeviceSpans(other, cases[0].table)
        rc, _, _ = ce.call(ctx, [(odev,) + wins[0][1:]], ops[:1], K_TOP, 8, check=False)
        assert rc == _lib.MR_ERR_ARG
        odev.close()
    finally:
        other.close()
    good()
    # MR_ERR_STATE: a time window on per-span window times; a trace shard of a larger table (global row
    # indices uploaded with it); a table without the per-trace index (an empty table is never indexed: no
    # edge dictionary), under the whole-table window and under a time window -- the missing index is
    # named, not the times it would have computed; a table without time columns, whole-table window
    # included.  The message names which.  (The refusals of a join of 2^32 pairs or 2^31 distinct edges
    # cannot be built at test sizes: such a table has more than 2^31 rows or 2^32 pairs.)
    import dataclasses

    st, _, c, t0, t1 = wx.table("span_times")
    full = cases[0].table
    shard = full.shard(0, 2)
    assert shard.row is not None and 0 < shard.n_spans < full.n_spans
    none = full.take(np.zeros(0, np.int64))
    assert none.n_spans == 0 and none.n_podops == full.n_podops
    timeless = dataclasses.replace(full, tstart=None, tend=None)
    whole = (ce.I64_MIN, ce.I64_MAX)
    for table, win, asked, word in ((st, None, [0, 1], "trace-level times"), (shard, None, [0, 1], "trace shard"),
                                    (none, whole, [], "edge dictionary"), (none, (0, 1), [], "edge dictionary"),
                                    (timeless, whole, [0, 1], "startTime/endTime"),
                                    (timeless, (0, 1), [0, 1], "startTime/endTime")):
        dev = DeviceSpans(ctx, table)
        try:
            a3, ok = np.full(table.n_svcops, 1.0), np.ones(table.n_svcops, np.uint8)
            w0, w1 = win if win is not None else (int(table.tstart.min()), int(table.tend.max()))
            rc, _, _ = ce.call(ctx, [(dev, w0, w1, a3, ok)], [asked], 2, 4, check=False)
            assert rc == _lib.MR_ERR_STATE, word
            assert word in _lib.load().mr_last_error(ctx.h).decode(), word
        finally:
            dev.close()
        good()


# ---------------------------------------------------------------------------------- the Python surface
def _entries(e, j, d, name=lambda c: c):
    n = int(e.n[j, d])
    return ([(name(int(e.peer[j, d, r])), int(e.calls[j, d, r, 1]), int(e.calls[j, d, r, 0]), int(e.dsum[j, d, r, 1]),
              int(e.dsum[j, d, r, 0]), int(e.dmax[j, d, r, 1]), int(e.dmax[j, d, r, 0])) for r in range(n)],
            int(e.peers[j, d]), (int(e.tot[j, d, 1]), int(e.tot[j, d, 0])))


def test_windows_call_edges_python(five):
    from microrank_amd.online_rca import windows_call_edges

    ctx, cases, wins = five
    asked = [ce.asked_ops(w) for w in cases]
    got = windows_call_edges(ctx, wins, asked, m=8)
    assert len(got) == len(cases)
    for w, a, g in zip(cases, asked, got):
        e = ce.expected(w.name, 8)
        assert list(g) == list(dict.fromkeys(a))
        for j, c in enumerate(a):
            assert g[c] == (_entries(e, j, 0), _entries(e, j, 1))
    assert windows_call_edges(ctx, [], []) == []


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden, regen_window

    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


def _named_oracle(adf, slo, operation_list, start, end, ops, m):
    """{op name: (callers, callees)} by names from the DataFrame's own factorisation and the reference
    detector's lists."""
    from microrank_amd.anormaly_detector import system_anomaly_detect
    from microrank_amd.spans import SpanTable

    with contextlib.redirect_stdout(io.StringIO()):
        flag, abnormal, normal = system_anomaly_detect(adf, start_time=start, end_time=end, slo=slo,
                                                       operation_list=operation_list)
    assert flag is True and abnormal and normal
    table = SpanTable.from_dataframe(adf)
    code = {n: i for i, n in enumerate(table.trace_names)}
    state = ce.kb.state_of(table.n_traces, [code[t] for t in abnormal], [code[t] for t in normal])
    pcode = {n: i for i, n in enumerate(table.podop_names)}
    asked = [pcode[o] for o in ops]
    e = ce.call_oracle(table, state, asked, max(len(asked), 1), m, int(pd.Timestamp(start).value), int(pd.Timestamp(end).value))
    name = lambda c: table.podop_names[c]
    return {key: (_entries(e, j, 0, name), _entries(e, j, 1, name)) for j, key in enumerate(ops)}


def test_rca_window_calls(golden):
    from microrank_amd.online_rca import rca_window

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo)
    assert plain["top"]
    with_calls = rca_window(adf, start, end, slo, call_edges=5)
    calls = with_calls.pop("calls")
    assert with_calls == plain                       # every other key is what it was
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 5)
    assert list(calls) == list(exp) and calls == exp
    assert sum(len(side[0]) for v in calls.values() for side in v) > 3


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


def test_driver_writes_calls_csv(golden, tmp_path, monkeypatch):
    c, adf, slo = golden
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_plain = _drive(adf, slo, c["operation_list"])
    assert os.path.exists("result.csv") and not os.path.exists("calls.csv")   # without the keyword: no file
    monkeypatch.chdir(tmp_path / "b")
    out_calls = _drive(adf, slo, c["operation_list"], call_edges=3)
    assert out_calls == out_plain
    assert open("result.csv", "rb").read() == open(tmp_path / "a" / "result.csv", "rb").read()
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    rows = list(csv.reader(open("calls.csv")))
    assert rows[0] == ["result", "rank", "direction", "peer", "calls_abnormal", "calls_normal", "mean_abnormal",
                       "mean_normal", "max_abnormal", "max_normal"]
    # the data holds one 5-minute window of traffic: the one trigger is the driver's first window
    start = adf["startTime"].min()
    exp = _named_oracle(adf, slo, c["operation_list"], start, start + pd.Timedelta(minutes=5), ranked, 3)
    want = [(r, str(rank), direction) + e for r in ranked for direction, side in zip(("caller", "callee"), exp[r])
            for rank, e in enumerate(side[0], start=1)]
    assert [tuple(x[:6]) for x in rows[1:]] == [w[:4] + (str(w[4]), str(w[5])) for w in want] and len(rows) > 4
    # the duration columns, not by the writer's own expression: a value of the file is in ms with four
    # decimals, so value * 1000 is within 0.05 duration units (half a step of 0.1) of the exact quotient of
    # the oracle's integers, plus the float64 rounding of a value of this size
    from fractions import Fraction

    some = 0
    for x, w in zip(rows[1:], want):
        _, _, _, _, ca, cn, sa, sn, xa, xn = w
        exact = [Fraction(sa, ca) if ca else Fraction(0), Fraction(sn, cn) if cn else Fraction(0), Fraction(xa), Fraction(xn)]
        for text, q in zip(x[6:], exact):
            v = float(text)
            assert repr(v) == text and round(v, 4) == v
            assert abs(Fraction(v) * 1000 - q) <= Fraction(5, 100) + abs(q) * Fraction(1, 10**12), (x, q)
            some += q != 0
    assert some > 8
    assert sorted(os.listdir(".")) == ["calls.csv", "result.csv"]
