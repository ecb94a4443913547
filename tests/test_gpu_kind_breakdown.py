"""GPU checks of mr_windows_kind_breakdown (csrc/mr_kind_breakdown.hip): per asked pod-op -- and for the
whole window -- the window's trace kinds with their abnormal and normal trace counts.  Every comparison
is exact integer equality of all nine outputs with the numpy oracle of tests/kind_breakdown_cases.py
(the span table's rows and oracle.detect's partition); no tolerance anywhere."""
import contextlib
import csv
import ctypes as C
import io
import os

import numpy as np
import pandas as pd
import pytest

import kind_breakdown_cases as kb
from kind_breakdown_cases import K_TOP

pytestmark = pytest.mark.gpu

NAMES = kb.WINDOWS + ("fault",)


@pytest.fixture(scope="module")
def five():
    """The five oracle windows on the device: (ctx, [window cases], [(DeviceSpans, t0, t1, a3, ok)])."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    cases = [kb.window(n) for n in NAMES]
    devs = [DeviceSpans(ctx, w.table) for w in cases]
    yield ctx, cases, [(d, w.t0, w.t1, w.a3, w.ok) for d, w in zip(devs, cases)]
    for d in devs:
        d.close()


def _one(ctx, w, asked, k, m):
    """One window on a table of its own: (outputs, status)."""
    from microrank_amd.preprocess_data import DeviceSpans

    dev = DeviceSpans(ctx, w.table)
    try:
        _, out, status = kb.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [asked], k, m)
    finally:
        dev.close()
    return out[0], status[0]


@pytest.mark.parametrize("m", kb.MS)
def test_oracle_equality_in_one_call_and_alone(five, m):
    ctx, cases, wins = five
    ops = [kb.asked_ops(w) for w in cases]
    assert any(len(o) == K_TOP for o in ops) and all(-1 in o and o.count(o[0]) == 2 for o in ops)
    _, out, status = kb.call(ctx, wins, ops, K_TOP, m)
    assert status.tolist() == [0] * len(wins)
    for w, o in zip(cases, out):
        kb.same(o, kb.expected(w.name, m))
    if m == 32:   # the padding: slots whose selected kinds number fewer than m
        e = kb.expected("ragged", m)
        assert ((e.n > 0) & (e.n < m)).any()
    for i, w in enumerate(cases):
        _, alone, st = kb.call(ctx, wins[i:i + 1], ops[i:i + 1], K_TOP, m)
        assert st.tolist() == [0] and kb.raw_bytes(alone) == kb.raw_bytes(out[i:i + 1]), w.name


def _boundary_ops(b):
    n = len(kb.BOUNDARY_SIZES)
    # every kind, the op all share, each kind's own op, two of the odd kinds' third ops, the dead kind's op
    return [-1, 0] + [i + 1 for i in range(n)] + [21, 23, n + 1]


@pytest.mark.parametrize("blocks", [None, "1", "7"])
def test_boundary_table(blocks, monkeypatch):
    from microrank_amd import _lib

    b = kb.boundary()
    live = kb.live_kinds(b.table, b.state, b.kinds)
    assert sorted(e[0] + e[1] for e in live) == sorted(kb.BOUNDARY_SIZES)        # the dead kind is not live
    assert all(e[0] > 0 and e[1] > 0 for e in live if e[0] + e[1] > 1)           # both sides in every kind
    asked = _boundary_ops(b)
    exp = kb.breakdown_oracle(b.table, b.state, asked, len(asked), 32, b.kinds)
    assert exp.kinds.tolist() == [10, 10] + [1] * 10 + [1, 1, 0]
    if blocks is not None:
        monkeypatch.setenv("MR_KB_BLOCKS", blocks)
    out, st = _one(_lib.default_context(), b, asked, len(asked), 32)
    assert st == 0
    kb.same(out, exp)


def test_window_of_20k_traces():
    """More than 20 build blocks of the layout; ~18.7k kinds, both sides populated."""
    from microrank_amd import _lib

    w = kb.big_window()
    assert w.table.n_traces == 20_000 and (w.state == 2).sum() > 5000 and (w.state == 1).sum() > 5000
    asked = kb.top_ops(w.table, w.state, K_TOP - 1) + [-1]
    assert len(asked) == K_TOP
    out, st = _one(_lib.default_context(), w, asked, K_TOP, 8)
    assert st == 0
    kb.same(out, kb.breakdown_oracle(w.table, w.state, asked, K_TOP, 8, w.kinds))


def test_invariance_under_blocks_chunks_and_order(five, monkeypatch):
    ctx, cases, wins = five
    ops = [kb.asked_ops(w) for w in cases]
    _, out, status = kb.call(ctx, wins, ops, K_TOP, 8)
    ref = kb.raw_bytes(out)
    for name, values in (("MR_KB_BLOCKS", ("1", "7")), ("MR_KB_CHUNK", ("1", "2"))):   # (both read per call)
        for v in values:
            monkeypatch.setenv(name, v)
            _, o, s = kb.call(ctx, wins, ops, K_TOP, 8)
            assert kb.raw_bytes(o) == ref and s.tolist() == status.tolist(), (name, v)
        monkeypatch.delenv(name)
    _, o, s = kb.call(ctx, wins[::-1], ops[::-1], K_TOP, 8)
    assert kb.raw_bytes(o[::-1]) == ref and s[::-1].tolist() == status.tolist()
    _, o, s = kb.call(ctx, wins, ops, K_TOP, 8)   # and twice the same
    assert kb.raw_bytes(o) == ref


def test_totals_equal_the_rankings_counts(five):
    from microrank_amd.online_rca import rank_windows

    ctx, cases, wins = five
    ranked = rank_windows(ctx, wins)
    _, out, _ = kb.call(ctx, wins, [[-1]] * len(wins), 1, 1)
    for w, r, o in zip(cases, ranked, out):
        assert (int(o.tot[0, 0]), int(o.tot[0, 1])) == (r[2], r[3]) == (int((w.state == 2).sum()), int((w.state == 1).sum()))


def test_empty_window_beside_a_good_one(five):
    from microrank_amd import _lib

    ctx, cases, wins = five
    ops = kb.asked_ops(cases[0])
    empty = (wins[0][0], 0, 1, wins[0][3], wins[0][4])   # no trace in [0, 1] ns
    _, out, status = kb.call(ctx, [empty, wins[0]], [ops, ops], K_TOP, 8)
    assert status.tolist() == [_lib.MR_ERR_VALUE, 0]
    kb.same(out[0], kb.breakdown_oracle(cases[0].table, None, ops, K_TOP, 8))
    kb.same(out[1], kb.expected(cases[0].name, 8))


def _wide_table():
    """4100 pod-ops (past the layout order's 4096) on 2050 traces of two rows, trace-level times."""
    from microrank_amd.spans import SpanTable

    nt = 2050
    tr = np.repeat(np.arange(nt, dtype=np.int32), 2)
    op = np.arange(2 * nt, dtype=np.int32)
    S = tr.size
    parent = np.where(np.arange(S) % 2 == 1, np.arange(S) - 1, -1).astype(np.int64)
    ts = np.repeat(np.arange(nt, dtype=np.int64) + 1000, 2)
    names = [f"pod_op{o:04d}" for o in range(2 * nt)]
    return SpanTable(tr, op, op.copy(), np.arange(S, dtype=np.int64), parent, np.full(S, 5000, np.int64), ts, ts + 10,
                     [f"t{i:04d}" for i in range(nt)], names, list(names))


def test_errors_leave_the_context_usable(five):
    import window_exemplar_cases as wx
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, wins = five
    ops = [kb.asked_ops(w) for w in cases]

    def good():
        _, out, status = kb.call(ctx, wins[:1], ops[:1], K_TOP, 8)
        assert status.tolist() == [0]
        kb.same(out[0], kb.expected(cases[0].name, 8))

    bad_calls = [
        dict(k=0), dict(k=65), dict(m=0), dict(m=33),
        dict(ops=[list(range(12))] + ops[1:]),                      # n_ops[i] outside 0..K
        dict(ops=[[0, cases[0].table.n_podops]] + ops[1:]),         # a code outside [-1, n_podops)
        dict(ops=[[0, -2]] + ops[1:]),
    ]
    for bad in bad_calls:
        kw = dict(wins=wins, ops=ops, k=K_TOP, m=8)
        kw.update(bad)
        rc, _, _ = kb.call(ctx, kw["wins"], kw["ops"], kw["k"], kw["m"], check=False)
        assert rc == _lib.MR_ERR_ARG, bad
        good()
    rc, _, _ = kb.call(ctx, wins, ops, K_TOP, 8, check=False, n_ops=[-1] + [len(o) for o in ops[1:]])   # n_ops[i] < 0
    assert rc == _lib.MR_ERR_ARG
    good()
    # a null pointer
    n1 = np.zeros(1, np.int32)
    rc = _lib.load().mr_windows_kind_breakdown(ctx.h, 1, None, None, None, None, None, None, _lib.ptr(n1, C.c_int32), 1, 1,
                                               None, None, None, None, None, None, None, None, None)
    assert rc == _lib.MR_ERR_ARG
    good()
    other = _lib.Context()   # a table of another context
    try:
        odev = DeviceSpans(other, cases[0].table)
        rc, _, _ = kb.call(ctx, [(odev,) + wins[0][1:]], ops[:1], K_TOP, 8, check=False)
        assert rc == _lib.MR_ERR_ARG
        odev.close()
    finally:
        other.close()
    good()
    # MR_ERR_STATE: per-span window times; a table past the layout limits; a trace shard of a larger table
    # (global row indices uploaded with it).  The message names which.
    st, _, c, t0, t1 = wx.table("span_times")
    shard = cases[0].table.shard(0, 2)
    assert shard.row is not None and 0 < shard.n_spans < cases[0].table.n_spans
    for table, word in ((st, "trace-level times"), (_wide_table(), "layout order"), (shard, "trace shard")):
        dev = DeviceSpans(ctx, table)
        try:
            a3, ok = np.full(table.n_svcops, 1.0), np.ones(table.n_svcops, np.uint8)
            rc, _, _ = kb.call(ctx, [(dev, int(table.tstart.min()), int(table.tend.max()), a3, ok)], [[-1, 0]], 2, 4,
                               check=False)
            assert rc == _lib.MR_ERR_STATE, word
            assert word in _lib.load().mr_last_error(ctx.h).decode(), word
        finally:
            dev.close()
        good()


# ---------------------------------------------------------------------------------- the Python surface
def test_windows_kind_breakdown_python(five):
    from microrank_amd.online_rca import windows_kind_breakdown

    ctx, cases, wins = five
    asked = [[None if c == -1 else c for c in kb.asked_ops(w)] for w in cases]
    got = windows_kind_breakdown(ctx, wins, asked, m=8)
    assert len(got) == len(cases)
    for w, a, g in zip(cases, asked, got):
        e = kb.expected(w.name, 8)
        assert list(g) == list(dict.fromkeys(a))
        for j, c in enumerate(a):
            entries, n_kinds, n_abn, n_nor = g[c]
            assert (n_kinds, n_abn, n_nor) == (int(e.kinds[j]), int(e.tot[j, 0]), int(e.tot[j, 1]))
            n = int(e.n[j])
            assert entries == list(zip(e.trace[j, :n].tolist(), e.abn[j, :n].tolist(), e.nor[j, :n].tolist(),
                                       e.spans[j, :n].tolist(), e.ops[j, :n].tolist()))
    assert windows_kind_breakdown(ctx, [], []) == []


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden, regen_window

    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


def _named_oracle(adf, slo, operation_list, start, end, ops, m):
    """{None / op name: (entries with trace names, n_kinds, n_abnormal, n_normal)} from the DataFrame's own
    factorisation and the reference detector's lists."""
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
    e = kb.breakdown_oracle(table, state, asked, len(asked), m)
    out = {}
    for j, key in enumerate([None] + list(ops)):
        n = int(e.n[j])
        out[key] = ([(table.trace_names[t], a, b, s, o) for t, a, b, s, o in
                     zip(e.trace[j, :n].tolist(), e.abn[j, :n].tolist(), e.nor[j, :n].tolist(), e.spans[j, :n].tolist(),
                         e.ops[j, :n].tolist())], int(e.kinds[j]), int(e.tot[j, 0]), int(e.tot[j, 1]))
    return out


def test_rca_window_kinds(golden):
    from microrank_amd.online_rca import rca_window

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo)
    assert plain["top"]
    with_kinds = rca_window(adf, start, end, slo, kind_breakdown=5)
    kinds = with_kinds.pop("kinds")
    assert with_kinds == plain                       # every other key is what it was
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 5)
    assert list(kinds) == list(exp) and kinds == exp
    assert kinds[None][2:] == (plain["n_abnormal"], plain["n_normal"])


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


def test_driver_writes_kinds_csv(golden, tmp_path, monkeypatch):
    c, adf, slo = golden
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_plain = _drive(adf, slo, c["operation_list"])
    assert os.path.exists("result.csv") and not os.path.exists("kinds.csv")   # without the keyword: no file
    monkeypatch.chdir(tmp_path / "b")
    out_kinds = _drive(adf, slo, c["operation_list"], kind_breakdown=3)
    assert out_kinds == out_plain
    assert open("result.csv", "rb").read() == open(tmp_path / "a" / "result.csv", "rb").read()
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    rows = list(csv.reader(open("kinds.csv")))
    assert rows[0] == ["result", "rank", "trace", "n_abnormal", "n_normal", "spans", "ops"]
    # the data holds one 5-minute window of traffic: the one trigger is the driver's first window
    start = adf["startTime"].min()
    exp = _named_oracle(adf, slo, c["operation_list"], start, start + pd.Timedelta(minutes=5), ranked, 3)
    want = []
    for label, key in [("*", None)] + [(r, r) for r in ranked]:
        for rank, e in enumerate(exp[key][0], start=1):
            want.append([label, str(rank)] + [str(x) for x in e])
    assert rows[1:] == want
    assert sum(r[0] == "*" for r in rows[1:]) == 3 and len(rows) > 4
