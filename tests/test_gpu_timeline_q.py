"""GPU checks of mr_windows_timeline_q (csrc/mr_timeline.hip): mr_windows_timeline's four integer outputs, byte for
byte, and np.quantile per (asked entry, bucket, side) of the values they count.  Every quantile is compared bit
for bit (float.hex) with the numpy oracle of tests/timeline_q_cases.py, or with mr_windows_latency's output; no
tolerance anywhere.  tests/test_timeline_q_cases.py checks on the CPU that the classes compared here are not
empty ones."""
import contextlib
import csv
import ctypes as C
import dataclasses
import io
import os

import numpy as np
import pandas as pd
import pytest

import call_edge_cases as ce
import kind_breakdown_cases as kb
import latency_cases as lc
import timeline_cases as tc
import timeline_q_cases as tq
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


@pytest.fixture(scope="module")
def boundary():
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    b = tc.boundary()
    dev = DeviceSpans(ctx, b.table)
    yield ctx, b, (dev, b.t0, b.t1, b.a3, b.ok)
    dev.close()


def _grids(cases, B, kind):
    g = [tc.grid(w, B, kind) for w in cases]
    return [x[0] for x in g], [x[1] for x in g]


def _last_error(ctx):
    from microrank_amd import _lib

    return _lib.load().mr_last_error(ctx.h).decode()


# ---------------------------------------------------------------------------------- the C entry
@pytest.mark.parametrize("B,what,method", tq.CASES, ids=lambda v: str(v))
def test_named_windows(five, B, what, method):
    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    b0, bw = _grids(cases, B, "default")
    _, out, status = tq.call(ctx, wins, ops, K_TOP, B, what, b0, bw, tq.QS, method)
    assert status.tolist() == [0] * len(wins)
    for w, o in zip(cases, out):
        exp, _ = tq.expected(w.name, B, what, method)
        assert o.q.shape == exp.shape and o.q.dtype == np.float64
        assert lc.hexes(o.q) == lc.hexes(exp), w.name
        tc.same(o, tc.expected(w.name, B, what))
    _, plain, pstatus = tc.call(ctx, wins, ops, K_TOP, B, what, b0, bw)
    assert tc.raw_bytes(out) == tc.raw_bytes(plain) and status.tolist() == pstatus.tolist()


def test_off_centre_grid_leaves_the_outside_rows_without_quantiles(five):
    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    b0, bw = _grids(cases, 7, "off")
    _, out, _ = tq.call(ctx, wins, ops, K_TOP, 7, "self", b0, bw)
    for w, o in zip(cases, out):
        assert lc.hexes(o.q) == lc.hexes(tq.expected(w.name, 7, "self", "linear", "off")[0]), w.name
        tc.same(o, tc.expected(w.name, 7, "self", "off"))
        assert o.out.any()


def _windows_latency(ctx, wins, ops, what, qs, method):
    """mr_windows_latency over ops: (out[n, K_TOP, 2, n_q], count[n, K_TOP, 2])."""
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
    qv = np.array(qs, np.float64)
    out = np.full((n, K_TOP, 2, qv.size), -7.5)
    cnt, status = np.full((n, K_TOP, 2), -7, np.int64), np.zeros(n, np.int32)
    ctx.check(_lib.load().mr_windows_latency(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                             ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), K_TOP, lc.WHAT[what],
                                             ptr(qv, C.c_double), qv.size, lc.METHODS[method], ptr(out, C.c_double),
                                             ptr(cnt, C.c_int64), ptr(status, C.c_int32)), "mr_windows_latency")
    return out, cnt


@pytest.mark.parametrize("what", tc.WHATS)
def test_one_bucket_equals_windows_latency(five, what):
    """B = 1 on the default grid: a pod-op slot's two classes are mr_windows_latency's, with no oracle in between."""
    ctx, cases, wins = five
    only = [[c for c in tc.asked_ops(w) if c >= 0] for w in cases]
    b0, bw = _grids(cases, 1, "default")
    some = 0
    for method in tq.METHODS:
        lat, count = _windows_latency(ctx, wins, only, what, tq.QS, method)
        _, out, _ = tq.call(ctx, wins, only, K_TOP, 1, what, b0, bw, tq.QS, method)
        for i, w in enumerate(cases):
            assert out[i].cnt[:, 0].tolist() == count[i].tolist() and not out[i].out.any(), (w.name, method)
            assert lc.hexes(out[i].q[:, 0]) == lc.hexes(lat[i]), (w.name, method)
            some += int((count[i] > 0).sum())
    assert some > 100


@pytest.mark.parametrize("grid", ["main", "ns"])
def test_boundary_table(boundary, grid):
    """Runs of BOUNDARY_SIZES consecutive rows of one class, two ops interleaved row by row, an op of negative
    values only (vmin < 0), an op without a row, rows on the edges of the bucket range, -1 and EDGE asked twice:
    boundary_ops() minus WRAP by duration -- and by self time, where WRAP's parent PAR is as wide and left out too."""
    ctx, b, win = boundary
    b0, bw, B = tc.GRIDS[grid]
    for what in tc.WHATS:
        asked, keep = tq.boundary_asked(what), tq.boundary_kept(what)
        assert tc.NEG in asked and tc.NEVER in asked and asked.count(-1) == 2 and asked.count(tc.EDGE) == 2
        assert tc.WRAP not in asked and (tc.PAR in asked) == (what == "duration")
        for method in tq.METHODS:
            _, out, st = tq.call(ctx, [win], [asked], len(asked), B, what, [b0], [bw], tq.QS, method)
            assert st.tolist() == [0]
            exp, cnt = tq.boundary_expected(grid, what, method)
            assert lc.hexes(out[0].q) == lc.hexes(exp), (what, method)
            e = tc.boundary_expected(grid, what)
            assert out[0].cnt.tolist() == cnt.tolist() == e.cnt[keep].tolist()
            assert out[0].sum.tolist() == e.sum[keep].tolist() and out[0].max.tolist() == e.max[keep].tolist()
            assert out[0].out.tolist() == e.out[keep].tolist()
    neg = tq.boundary_asked("duration").index(tc.NEG)   # (its trace starts inside `main`, after the end of `ns`)
    assert (tq.boundary_expected("main", "duration", "linear")[0][neg] < 0).any()


def test_value_range_too_wide(boundary):
    """WRAP's values span 2^63: no 64-bit key holds them beside a class.  MR_ERR_ARG naming the range; the context
    stays usable, and the plain entry still answers the same call."""
    from microrank_amd import _lib

    ctx, b, win = boundary
    b0, bw, B = tc.GRIDS["main"]
    asked = tc.boundary_ops()
    rc, _, _ = tq.call(ctx, [win], [asked], len(asked), B, "duration", [b0], [bw], check=False)
    assert rc == _lib.MR_ERR_ARG
    msg = _last_error(ctx)
    assert "mr_windows_timeline_q" in msg and "value range too wide" in msg and str(-tc.BIG - 10) in msg, msg
    # PAR, WRAP's parent: by duration it fits, by self time (100 minus the children's) it is as wide as WRAP
    only_par = [tc.PAR, -1]
    rc, _, _ = tq.call(ctx, [win], [only_par], 2, B, "self", [b0], [bw], check=False)
    assert rc == _lib.MR_ERR_ARG and "value range too wide" in _last_error(ctx), _last_error(ctx)
    _, out, st = tq.call(ctx, [win], [only_par], 2, B, "duration", [b0], [bw])
    assert st.tolist() == [0] and out[0].cnt[0].sum() > 0
    good = tq.boundary_asked("duration")
    _, out, st = tq.call(ctx, [win], [good], len(good), B, "duration", [b0], [bw])
    assert st.tolist() == [0] and lc.hexes(out[0].q) == lc.hexes(tq.boundary_expected("main", "duration", "linear")[0])
    _, plain, _ = tc.call(ctx, [win], [asked], len(asked), B, "duration", [b0], [bw])
    tc.same(plain[0], tc.boundary_expected("main", "duration"))


def test_cuts_give_identical_bytes(five, monkeypatch):
    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    for B, kind in ((30, "off"), (512, "default")):
        b0, bw = _grids(cases, B, kind)
        _, out, status = tq.call(ctx, wins, ops, K_TOP, B, "self", b0, bw)
        ref = tq.raw_bytes(out)
        assert any(o.q.any() for o in out)
        for name, values in (("MR_TL_CHUNK", ("1", "3")), ("MR_TL_BLOCKS", ("1", "2", "7"))):   # (both read per call)
            for v in values:
                monkeypatch.setenv(name, v)
                _, o, s = tq.call(ctx, wins, ops, K_TOP, B, "self", b0, bw)
                assert tq.raw_bytes(o) == ref and s.tolist() == status.tolist(), (name, v)
            monkeypatch.delenv(name)
        monkeypatch.setenv("MR_TL_CHUNK", "3")
        monkeypatch.setenv("MR_TL_BLOCKS", "2")
        _, o, _ = tq.call(ctx, wins, ops, K_TOP, B, "self", b0, bw)
        assert tq.raw_bytes(o) == ref
        monkeypatch.delenv("MR_TL_CHUNK")
        monkeypatch.delenv("MR_TL_BLOCKS")


def test_many_windows_in_one_call(five):
    """Eight windows over two tables, an empty window and a window with n_ops = 0 among them: each equals the
    window alone, and a window moved to another place in the call keeps its bytes."""
    from microrank_amd import _lib

    ctx, cases, wins = five
    a, f = 0, NAMES.index("fault")
    B = 7
    ga, gf = tc.grid(cases[a], B), tc.grid(cases[f], B, "off")
    oa, of = tc.asked_ops(cases[a]), tc.asked_ops(cases[f])
    empty = (wins[a][0], 0, 1, wins[a][3], wins[a][4])   # no trace in [0, 1] ns
    call = [(wins[a], oa, ga), (wins[f], of, gf), (empty, oa, (0, 1)), (wins[f], [], gf), (wins[a], oa[::-1], ga),
            (wins[f], of[:3], gf), (wins[a], [-1], ga), (wins[f], of, gf)]

    def run(items):
        _, out, st = tq.call(ctx, [x[0] for x in items], [x[1] for x in items], K_TOP, B, "self", [x[2][0] for x in items],
                             [x[2][1] for x in items])
        return out, st.tolist()

    out, status = run(call)
    assert status == [0, 0, _lib.MR_ERR_VALUE, 0, 0, 0, 0, 0]
    assert not out[2].q.any() and not out[2].cnt.any() and not out[3].q.any() and not out[3].cnt.any()
    assert lc.hexes(out[0].q) == lc.hexes(tq.expected(NAMES[a], B, "self", "linear")[0])
    assert lc.hexes(out[1].q) == lc.hexes(tq.expected("fault", B, "self", "linear", "off")[0])
    assert out[7].q.any() and tq.raw_bytes(out[7:8]) == tq.raw_bytes(out[1:2])
    for i, item in enumerate(call):
        alone, st = run([item])
        assert st == [status[i]] and tq.raw_bytes(alone) == tq.raw_bytes(out[i:i + 1]), i
    moved = call[1:] + call[:1]
    out2, status2 = run(moved)
    assert status2 == status[1:] + status[:1] and tq.raw_bytes(out2) == tq.raw_bytes(out[1:] + out[:1])


def test_argument_errors_leave_the_context_usable(five):
    from microrank_amd import _lib

    ctx, cases, wins = five
    ops = [tc.asked_ops(w) for w in cases]
    b0, bw = _grids(cases, 7, "default")

    def good():
        _, out, status = tq.call(ctx, wins[:1], ops[:1], K_TOP, 7, "self", b0[:1], bw[:1])
        assert status.tolist() == [0]
        assert lc.hexes(out[0].q) == lc.hexes(tq.expected(cases[0].name, 7, "self", "linear")[0])

    for bad in (dict(qs=[1.5]), dict(qs=[-0.1]), dict(qs=[0.5, float("nan")]), dict(n_q=0), dict(n_q=17), dict(method=3),
                dict(method=-1), dict(what=2), dict(B=0), dict(B=513), dict(k=0), dict(k=65), dict(bw=[0] + bw[1:])):
        kw = dict(k=K_TOP, B=7, what="self", bw=bw, qs=tq.QS, method="linear", n_q=None)
        kw.update(bad)
        rc, _, _ = tq.call(ctx, wins, ops, kw["k"], kw["B"], kw["what"], b0, kw["bw"], kw["qs"], kw["method"], check=False,
                           n_q=kw["n_q"])
        assert rc == _lib.MR_ERR_ARG, bad
        assert "mr_windows_timeline_q" in _last_error(ctx)
        good()


def test_not_covered_states(five):
    """MR_ERR_STATE with mr_windows_timeline's list, order and messages (tests/test_gpu_timeline.py)."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, _ = five
    timeless = lc.banded_table(times=False)[0]
    st = ce.window("span_times").table
    full = cases[0].table
    shard = full.shard(0, 2)
    none = full.take(np.zeros(0, np.int64))
    timeless_shard = dataclasses.replace(shard, tstart=None, tend=None)
    whole = (tc.I64_MIN, tc.I64_MAX)
    for table, win, asked, what, word in ((timeless, whole, [0, -1], "self", "startTime/endTime"),
                                          (timeless_shard, whole, [0, -1], "self", "startTime/endTime"),
                                          (st, None, [0], "duration", "trace-level times"),
                                          (shard, None, [0, -1], "self", "self time on a trace shard"),
                                          (shard, None, [0, -1], "duration", "slot -1 on a trace shard"),
                                          (none, (0, 1), [-1], "duration", "per-trace index")):
        dev = DeviceSpans(ctx, table)
        try:
            a3, ok = np.full(table.n_svcops, 1.0), np.ones(table.n_svcops, np.uint8)
            w0, w1 = win if win is not None else (int(table.tstart.min()), int(table.tend.max()))
            rc, _, _ = tq.call(ctx, [(dev, w0, w1, a3, ok)], [asked], 2, 4, what, [0], [1000], check=False)
            assert rc == _lib.MR_ERR_STATE, word
            msg = _last_error(ctx)
            assert word in msg and msg.startswith("mr_windows_timeline_q:"), msg
            rc2, _, _ = tc.call(ctx, [(dev, w0, w1, a3, ok)], [asked], 2, 4, what, [0], [1000], check=False)
            assert rc2 == rc and _last_error(ctx) == msg.replace("mr_windows_timeline_q:", "mr_windows_timeline:")
        finally:
            dev.close()


def test_op_slots_on_a_trace_shard(five):
    """Op slots with MR_LAT_DURATION on a trace shard are allowed, as in mr_windows_timeline: that rank's rows."""
    import oracle as orc
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, _ = five
    w = cases[0]
    shard = w.table.shard(1, 2)
    res = orc.detect(shard.trace, shard.svcop, shard.duration, shard.tstart, shard.tend, w.t0, w.t1,
                     {i: float(w.a3[i]) for i in range(w.a3.size) if w.ok[i]})
    state = kb.state_of(shard.n_traces, res[1], res[2])
    asked = [c for c in tc.asked_ops(w) if c >= 0]
    b0, bw = tc.grid(w, 7)
    dev = DeviceSpans(ctx, shard)
    try:
        _, out, status = tq.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [asked], K_TOP, 7, "duration", [b0], [bw])
    finally:
        dev.close()
    exp, cnt = tq.quantile_oracle(shard, state, asked, K_TOP, 7, "duration", b0, bw, tq.QS, "linear", w.t0, w.t1)
    assert status.tolist() == [0] and cnt.sum() > 0
    assert lc.hexes(out[0].q) == lc.hexes(exp) and out[0].cnt.tolist() == cnt.tolist()


# ---------------------------------------------------------------------------------- the Python surface
def test_windows_timeline_q_python(five):
    from microrank_amd.online_rca import windows_timeline, windows_timeline_q

    ctx, cases, wins = five
    asked = [tc.asked_ops(w) for w in cases]
    got = windows_timeline_q(ctx, wins, asked, q=(0.5, 0.99), buckets=30, what="duration", method="higher")
    plain = windows_timeline(ctx, wins, asked, buckets=30, what="duration")
    qi = [tq.QS.index(0.5), tq.QS.index(0.99)]
    for w, a, g, p in zip(cases, asked, got, plain):
        exp, _ = tq.expected(w.name, 30, "duration", "higher")
        assert list(g) == list(dict.fromkeys(a))
        for j, c in enumerate(a):
            assert sorted(g[c]) == sorted(list(p[c]) + ["q", "quantile"])
            assert all(g[c][k].tolist() == p[c][k].tolist() and g[c][k].dtype == p[c][k].dtype for k in p[c])
            assert g[c]["q"].dtype == np.float64 and g[c]["q"].tolist() == [0.5, 0.99]
            assert g[c]["quantile"].dtype == np.float64 and g[c]["quantile"].shape == (30, 2, 2)
            assert lc.hexes(g[c]["quantile"]) == lc.hexes(exp[j][:, :, qi])
    one = windows_timeline_q(ctx, wins[:1], asked[:1], q=0.5, buckets=7)[0]
    assert one[-1]["quantile"].shape == (7, 2, 1)
    assert windows_timeline_q(ctx, [], []) == []


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden, regen_window

    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


Q2 = (0.5, 0.99)


def _named_oracle(adf, slo, operation_list, start, end, ops, B, what, qs=Q2):
    """{-1 / op name: window_timeline_q's lists} by names from the DataFrame's own factorisation and the reference
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
    e = tc.timeline_oracle(table, state, asked, len(asked), B, what, b0, bw, t0, t1)
    q, cnt = tq.quantile_oracle(table, state, asked, len(asked), B, what, b0, bw, qs, "linear", t0, t1)
    assert cnt.tolist() == e.cnt.tolist()
    return {key: {"start": [b0 + b * bw for b in range(B)], "cnt": e.cnt[j].tolist(), "sum": e.sum[j].tolist(),
                  "max": e.max[j].tolist(), "out": e.out[j].tolist(), "q": list(qs), "quantile": q[j].tolist()}
            for j, key in enumerate([-1] + list(ops))}


def test_rca_window_timeline_q(golden):
    from microrank_amd.online_rca import rca_window, window_timeline, window_timeline_q

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo, timeline=6)
    got = rca_window(adf, start, end, slo, timeline=6, timeline_q=Q2)
    tl = got.pop("timeline")
    old = plain.pop("timeline")
    assert got == plain and old == window_timeline(adf, start, end, slo, plain["top"], buckets=6)
    assert tl == window_timeline_q(adf, start, end, slo, plain["top"], q=Q2, buckets=6)
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 6, "self")
    assert list(tl) == list(exp) and tl == exp
    assert {k: v for k, v in tl[-1].items() if k not in ("q", "quantile")} == old[-1]
    dur = rca_window(adf, start, end, slo, timeline=6, timeline_q=Q2, timeline_what="duration")["timeline"]
    assert dur == _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 6, "duration") and dur != tl
    only_what = rca_window(adf, start, end, slo, timeline=6, timeline_what="duration")["timeline"]
    assert only_what == {k: {f: v[f] for f in old[-1]} for k, v in dur.items()}


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


def _written(path, write, *args):
    """The files ``write(*args)`` leaves in a fresh directory: {name: bytes}."""
    cwd = os.getcwd()
    os.makedirs(path)
    os.chdir(path)
    try:
        write(*args)
        return {n: open(n, "rb").read() for n in sorted(os.listdir("."))}
    finally:
        os.chdir(cwd)


def test_driver_writes_timeline_q_csv(golden, tmp_path, monkeypatch):
    from microrank_amd import online_rca as o

    c, adf, slo = golden
    for d in "abcde":
        (tmp_path / d).mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_tl = _drive(adf, slo, c["operation_list"], timeline=6)
    assert sorted(os.listdir(".")) == ["result.csv", "timeline.csv"]   # without timeline_q: the files of today
    monkeypatch.chdir(tmp_path / "b")
    out_q = _drive(adf, slo, c["operation_list"], timeline=6, timeline_q=Q2)   # the sweep path
    assert out_q == out_tl and sorted(os.listdir(".")) == ["result.csv", "timeline.csv", "timeline_q.csv"]
    for name in ("result.csv", "timeline.csv"):
        assert open(name, "rb").read() == open(tmp_path / "a" / name, "rb").read(), name
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    rows = list(csv.reader(open("timeline_q.csv")))
    assert rows[0] == ["result", "rank", "bucket", "start", "side", "spans", "q", "value"]
    # the data holds one 5-minute window of traffic: the one trigger is the driver's first window
    start = adf["startTime"].min()
    end = start + pd.Timedelta(minutes=5)
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, ranked, 6, "self")
    want = [[label, str(rank), str(b), str(e["start"][b]), side, str(e["cnt"][b][s]), repr(float(qj)),
             repr(float(np.round(np.float64(e["quantile"][b][s][k]) / 1000.0, 4)))]
            for rank, (label, e) in enumerate([("*", exp[-1])] + [(r, exp[r]) for r in ranked]) for b in range(6)
            for s, side in enumerate(("normal", "abnormal")) for k, qj in enumerate(Q2)]
    assert rows[1:] == want and len(ranked) > 2
    assert sum(float(x[7]) != 0.0 for x in rows[1:]) > 20 and all(x[7] == "0.0" for x in rows[1:] if x[5] == "0")
    # the window-by-window fallback writes the same files
    evidence = o.evidence_request(timeline=6, timeline_q=Q2)
    monkeypatch.chdir(tmp_path / "c")
    with contextlib.redirect_stdout(io.StringIO()):
        o._window_loop(adf.copy(), slo, c["operation_list"], start, adf["endTime"].max(), 25, evidence)
    assert sorted(os.listdir(".")) == ["result.csv", "timeline.csv", "timeline_q.csv"]
    for name in ("timeline.csv", "timeline_q.csv"):
        assert open(name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    # and so does the stream
    monkeypatch.chdir(tmp_path / "d")
    with contextlib.redirect_stdout(io.StringIO()):
        s = o.RCAStream(slo, c["operation_list"], timeline=6, timeline_q=Q2)
        s.push(adf.copy())
        s.close()
    for name in ("timeline.csv", "timeline_q.csv"):
        assert open(name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    # timeline_what="duration": timeline.csv is the duration oracle's
    monkeypatch.chdir(tmp_path / "e")
    assert _drive(adf, slo, c["operation_list"], timeline=6, timeline_what="duration") == out_tl
    assert sorted(os.listdir(".")) == ["result.csv", "timeline.csv"]
    dur = _named_oracle(adf, slo, c["operation_list"], start, end, ranked, 6, "duration")
    plain_rows = {k: {f: v[f] for f in ("start", "cnt", "sum", "max", "out")} for k, v in dur.items()}
    scores = [float(len(ranked) - i) for i in range(len(ranked))]
    want_files = _written(str(tmp_path / "want"), o._write_timeline, ranked, scores, plain_rows)
    assert list(want_files) == ["timeline.csv"] and open("timeline.csv", "rb").read() == want_files["timeline.csv"]
    assert want_files["timeline.csv"] != open(tmp_path / "a" / "timeline.csv", "rb").read()
