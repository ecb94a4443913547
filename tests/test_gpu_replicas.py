"""GPU checks of mr_windows_replicas (csrc/mr_replicas.hip): per asked pod-op the pod-ops of its service-op --
its replicas -- with the count, the summed and the largest value of their rows on each side of the window's
detector partition, the first m under the order, the op's own numbers and place, and the service-op's totals.
Every comparison is exact integer equality of all ten outputs with the numpy oracle of tests/replica_cases.py
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
import latency_cases as lc
import replica_cases as rc
import timeline_cases as tc

pytestmark = pytest.mark.gpu

NAMES = tuple(rc.CASES)


def _k_all():
    """K of the calls over all four cases: the longest asked list (the cases are built on first use)."""
    return max(len(rc.asked(n)) for n in NAMES)


@pytest.fixture(scope="module")
def four():
    """The four named cases on the device: (ctx, [cases], [(DeviceSpans, t0, t1, a3, ok)])."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    cases = [rc.CASES[n]() for n in NAMES]
    devs = [DeviceSpans(ctx, w.table) for w in cases]
    yield ctx, cases, [(d, w.t0, w.t1, w.a3, w.ok) for d, w in zip(devs, cases)]
    for d in devs:
        d.close()


@pytest.mark.parametrize("what", rc.WHATS)
@pytest.mark.parametrize("m", rc.MS)
def test_oracle_equality_in_one_call_and_alone(four, m, what):
    ctx, cases, wins = four
    ops = [rc.asked(n) for n in NAMES]
    k = _k_all()
    _, out, status = rc.call(ctx, wins, ops, k, m, what)
    assert status.tolist() == [0] * len(wins)
    for n, o in zip(NAMES, out):
        rc.same(o, rc.expected(n, m, what, k))
    for i, n in enumerate(NAMES):
        _, alone, st = rc.call(ctx, wins[i:i + 1], ops[i:i + 1], k, m, what)
        assert st.tolist() == [0] and rc.raw_bytes(alone) == rc.raw_bytes(out[i:i + 1]), n


def test_one_pod_asked_by_its_sibling(four):
    """The fault op's abnormal rows all on pod 0 (code 115), asked by pod 1 (117): the answer says "it is that pod"."""
    ctx, cases, wins = four
    i = NAMES.index("one_pod")
    _, out, st = rc.call(ctx, [wins[i]], [[117]], 1, 8, "self")
    o = out[0]
    assert st.tolist() == [0] and o.pod[0, :4].tolist() == [115, 119, 117, -1]
    assert o.cnt[0, :3, ::-1].tolist() == [[228, 438], [0, 415], [0, 433]]      # (abnormal, normal)
    assert (int(o.place[0]), int(o.live[0]), int(o.all[0]), int(o.n[0])) == (2, 3, 3, 3)


@pytest.mark.parametrize("blocks", ["1", "7"])
def test_boundary_table(four, blocks, monkeypatch):
    ctx, cases, wins = four
    i = NAMES.index("boundary")
    ops = rc.boundary_ops()
    monkeypatch.setenv("MR_RP_BLOCKS", blocks)
    for what in rc.WHATS:
        for m in (2, 32):
            _, out, st = rc.call(ctx, [wins[i]], [ops], len(ops), m, what)
            assert st.tolist() == [0]
            rc.same(out[0], rc.expected("boundary", m, what))


def test_invariance_under_blocks_chunks_and_order(four, monkeypatch):
    ctx, cases, wins = four
    ops = [rc.asked(n) for n in NAMES]
    k = _k_all()
    _, out, status = rc.call(ctx, wins, ops, k, 8, "self")
    ref = rc.raw_bytes(out)
    for name, values in (("MR_RP_BLOCKS", ("1", "7")), ("MR_RP_CHUNK", ("1", "2"))):   # (both read per call)
        for v in values:
            monkeypatch.setenv(name, v)
            _, o, s = rc.call(ctx, wins, ops, k, 8, "self")
            assert rc.raw_bytes(o) == ref and s.tolist() == status.tolist(), (name, v)
        monkeypatch.delenv(name)
    _, o, s = rc.call(ctx, wins[::-1], ops[::-1], k, 8, "self")
    assert rc.raw_bytes(o[::-1]) == ref and s[::-1].tolist() == status.tolist()
    _, o, s = rc.call(ctx, wins, ops, k, 8, "self")   # and twice the same
    assert rc.raw_bytes(o) == ref


def test_direct_against_hashed(four):
    """`wide` asked with 5 slots (<= 1024 keys: the block's table is direct-mapped) and with 12 (hashed) agrees on
    the common entries."""
    ctx, cases, wins = four
    i = NAMES.index("wide")
    w = cases[i]
    ops = rc.wide_ops(w)
    sv, _ = rc.sv_map(w.table)
    assert sum(int((sv == sv[p]).sum()) for p in ops[:5]) * 2 <= 1024 < sum(int((sv == sv[p]).sum()) for p in ops) * 2
    _, five, _ = rc.call(ctx, [wins[i]], [ops[:5]], 12, 32, "self")
    _, twelve, _ = rc.call(ctx, [wins[i]], [ops], 12, 32, "self")
    for f in rc.FIELDS:
        assert getattr(five[0], f)[:5].tolist() == getattr(twelve[0], f)[:5].tolist(), f
    rc.same(twelve[0], rc.replica_oracle(w.table, w.state, ops, 12, 32, "self", w.t0, w.t1))
    h = rc.wide(half=True)   # the first half of the time range: live < all
    _, out, st = rc.call(ctx, [(wins[i][0], h.t0, h.t1, h.a3, h.ok), wins[i]], [ops, ops], 12, 32, "self")
    assert st.tolist() == [0, 0]
    rc.same(out[0], rc.replica_oracle(w.table, h.state, ops, 12, 32, "self", h.t0, h.t1))
    assert (out[0].live < out[0].all).all() and rc.raw_bytes(out[1:]) == rc.raw_bytes(twelve)


def _windows_latency(ctx, win, codes, what):
    """mr_windows_latency's count[len(codes), 2] of one window."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    k = len(codes)
    spans = (_lib.P * 1)(win[0].h)
    t0, t1 = np.array([win[1]], np.int64), np.array([win[2]], np.int64)
    a3, ok = (C.c_void_p * 1)(win[3].ctypes.data), (C.c_void_p * 1)(win[4].ctypes.data)
    cod, n_ops = np.array([codes], np.int32), np.array([k], np.int32)
    qv = np.array([0.5], np.float64)
    out, cnt, status = np.zeros((1, k, 2, 1)), np.zeros((1, k, 2), np.int64), np.zeros(1, np.int32)
    ctx.check(_lib.load().mr_windows_latency(ctx.h, 1, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                             ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, lc.WHAT[what],
                                             ptr(qv, C.c_double), 1, 0, ptr(out, C.c_double), ptr(cnt, C.c_int64),
                                             ptr(status, C.c_int32)), "mr_windows_latency")
    return cnt[0]


def test_cross_checks_against_the_shipped_entries(four):
    """Every listed replica and side: (cnt, sum, max) == mr_windows_timeline's one bucket over everything when the
    replica is asked there as an op, cnt == mr_windows_latency's count; rp_own is the entry at rp_place; with
    live <= m rp_tot is the entries' sums and maximum; every replica of one service-op, asked in turn, gets the
    same list and totals."""
    ctx, cases, wins = four
    i = NAMES.index("pods3")
    w, win = cases[i], wins[i]
    ops = rc.asked("pods3")
    k = len(ops)
    sv, _ = rc.sv_map(w.table)
    assert 0 <= w.table.tstart.min() and w.table.tstart.max() < tc.BIG
    for what in rc.WHATS:
        _, out, _ = rc.call(ctx, [win], [ops], k, 8, what)
        o = out[0]
        listed = sorted({int(q) for q in o.pod.reshape(-1) if q >= 0})
        assert 10 < len(listed) <= 64
        at = {q: j for j, q in enumerate(listed)}
        # B = 1 over [0, 2^62): one bucket that holds every start of this table
        _, one, _ = tc.call(ctx, [win], [listed], len(listed), 1, what, [0], [tc.BIG])
        count = _windows_latency(ctx, win, listed, what)
        assert not one[0].out.any()
        checked = 0
        for j in range(k):
            assert o.live[j] <= 8 and o.n[j] == o.live[j]
            for e in range(int(o.n[j])):
                q = at[int(o.pod[j, e])]
                assert o.cnt[j, e].tolist() == one[0].cnt[q, 0].tolist() == count[q].tolist()
                assert o.sum[j, e].tolist() == one[0].sum[q, 0].tolist() and o.max[j, e].tolist() == one[0].max[q, 0].tolist()
                checked += 1
            if 0 <= o.place[j] < o.n[j]:
                e = int(o.place[j])
                assert o.pod[j, e] == ops[j]
                assert o.own[j].tolist() == [[int(o.cnt[j, e, s]), int(o.sum[j, e, s]), int(o.max[j, e, s])] for s in (0, 1)]
            n = int(o.n[j])
            if n:
                with np.errstate(over="ignore"):
                    sums = o.sum[j, :n].sum(axis=0)
                for s in (0, 1):
                    on = [int(o.max[j, e, s]) for e in range(n) if o.cnt[j, e, s]]
                    assert o.tot[j, s].tolist() == [int(o.cnt[j, :n, s].sum()), int(sums[s]), max(on) if on else 0]
        assert checked > 30
        reps = [int(q) for q in rc.replicas_of(sv, sv[ops[0]])]     # one service-op's replicas in turn
        _, turn, _ = rc.call(ctx, [win], [reps], len(reps), 8, what)
        for j in range(1, len(reps)):
            for f in ("pod", "cnt", "sum", "max", "n", "live", "all", "tot"):
                assert getattr(turn[0], f)[j].tolist() == getattr(turn[0], f)[0].tolist(), f
        assert sorted(turn[0].place.tolist()) == list(range(len(reps)))


def test_empty_window_beside_a_good_one(four):
    from microrank_amd import _lib

    ctx, cases, wins = four
    ops = rc.asked("pods3")
    empty = (wins[0][0], 0, 1, wins[0][3], wins[0][4])   # no trace in [0, 1] ns
    _, out, status = rc.call(ctx, [empty, wins[0]], [ops, ops], len(ops), 8, "self")
    assert status.tolist() == [_lib.MR_ERR_VALUE, 0]
    rc.same(out[0], rc.replica_oracle(cases[0].table, None, ops, len(ops), 8, "self"))
    rc.same(out[1], rc.expected("pods3", 8, "self"))


def test_whole_table_window_of_per_span_times():
    """A whole-table window on a table whose times vary within a trace (the row-level detector) equals the oracle;
    a time window on it is MR_ERR_STATE."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    w = rc.span_times()
    ctx = _lib.default_context()
    ops = rc.top_by_abnormal_rows(w.table, w.state)
    ops = ops + [ops[0]]
    dev = DeviceSpans(ctx, w.table)
    try:
        whole = (dev, rc.I64_MIN, rc.I64_MAX, w.a3, w.ok)
        for what in rc.WHATS:
            _, out, st = rc.call(ctx, [whole, whole], [ops, ops[:3]], len(ops), 8, what)
            assert st.tolist() == [0, 0]
            exp = rc.replica_oracle(w.table, w.state, ops, len(ops), 8, what)   # (the case's window spans its table)
            assert exp.live.sum() > 0 and (exp.all == 2).all()
            rc.same(out[0], exp)
            rc.same(out[1], rc.replica_oracle(w.table, w.state, ops[:3], len(ops), 8, what))
        rcode, _, _ = rc.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [ops], len(ops), 8, "self", check=False)
        assert rcode == _lib.MR_ERR_STATE and "trace-level times" in lc.last_error(ctx)
    finally:
        dev.close()


def test_errors_leave_the_context_usable(four):
    import dataclasses

    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, wins = four
    ops = [rc.asked(n) for n in NAMES]
    k = _k_all()
    _, before, _ = rc.call(ctx, wins[:1], ops[:1], k, 8, "self")
    ref = rc.raw_bytes(before)

    def good():
        _, out, status = rc.call(ctx, wins[:1], ops[:1], k, 8, "self")
        assert status.tolist() == [0] and rc.raw_bytes(out) == ref
        rc.same(out[0], rc.expected("pods3", 8, "self", k))

    bad_calls = [
        dict(k=0), dict(k=65), dict(m=0), dict(m=33), dict(what=2), dict(what=-1),
        dict(ops=[list(range(k + 1))] + ops[1:]),                   # n_ops[i] outside 0..K
        dict(ops=[[0, cases[0].table.n_podops]] + ops[1:]),         # a code outside [0, n_podops)
        dict(ops=[[0, -1]] + ops[1:]),
    ]
    for bad in bad_calls:
        kw = dict(ops=ops, k=k, m=8, what="self")
        kw.update(bad)
        rcode, _, _ = rc.call(ctx, wins, kw["ops"], kw["k"], kw["m"], kw["what"], check=False)
        assert rcode == _lib.MR_ERR_ARG, bad
        good()
    rcode, _, _ = rc.call(ctx, wins, ops, k, 8, "self", check=False, n_ops=[-1] + [len(o) for o in ops[1:]])
    assert rcode == _lib.MR_ERR_ARG
    good()
    n1 = np.zeros(1, np.int32)   # a null pointer
    rcode = _lib.load().mr_windows_replicas(ctx.h, 1, None, None, None, None, None, None, _lib.ptr(n1, C.c_int32), 1, 1, 0,
                                            None, None, None, None, None, None, None, None, None, None, None)
    assert rcode == _lib.MR_ERR_ARG
    good()
    other = _lib.Context()   # a table of another context
    try:
        odev = DeviceSpans(other, cases[0].table)
        rcode, _, _ = rc.call(ctx, [(odev,) + wins[0][1:]], ops[:1], k, 8, "self", check=False)
        assert rcode == _lib.MR_ERR_ARG
        odev.close()
    finally:
        other.close()
    good()
    # MR_ERR_STATE, in the header's order; the message names the case
    full = cases[0].table
    timeless = dataclasses.replace(full, tstart=None, tend=None)
    shard = full.shard(0, 2)
    assert shard.row is not None and 0 < shard.n_spans < full.n_spans
    a = rc.ambiguous()
    whole = (rc.I64_MIN, rc.I64_MAX)
    for table, win, what, words in ((timeless, whole, "self", ["startTime/endTime"]),
                                    (dataclasses.replace(a.table, tstart=None, tend=None), whole, "self", ["startTime/endTime"]),
                                    (shard, None, "self", ["self time on a trace shard"]),
                                    (a.table, None, "self", ["ambiguous", f"pod-op {a.pod} ", f"service-op {a.svcs[0]} ",
                                                             f"service-op {a.svcs[1]} "]),
                                    (a.table, None, "duration", ["ambiguous", f"pod-op {a.pod} "])):
        dev = DeviceSpans(ctx, table)
        try:
            w0, w1 = win if win is not None else (cases[0].t0, cases[0].t1)
            for _ in range(2):   # (an ambiguous table keeps its verdict: the second call fails without a rebuild)
                rcode, _, _ = rc.call(ctx, [(dev, w0, w1, cases[0].a3, cases[0].ok)], [ops[0]], k, 8, what, check=False)
                assert rcode == _lib.MR_ERR_STATE, words
                for word in words:
                    assert word in lc.last_error(ctx), word
        finally:
            dev.close()
        good()


def test_trace_shard(four):
    """MR_LAT_DURATION on a 2-way trace shard covers that rank's rows and that rank's map -- the oracle on the
    shard's own table; MR_LAT_SELF there is MR_ERR_STATE."""
    import oracle as orc
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx, cases, _ = four
    w = cases[0]
    shard = w.table.shard(1, 2)
    res = orc.detect(shard.trace, shard.svcop, shard.duration, shard.tstart, shard.tend, w.t0, w.t1,
                     {i: float(w.a3[i]) for i in range(w.a3.size) if w.ok[i]})
    state = kb.state_of(shard.n_traces, res[1], res[2])
    ops = rc.asked("pods3")
    dev = DeviceSpans(ctx, shard)
    try:
        _, out, status = rc.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [ops], len(ops), 8, "duration")
        rcode, _, _ = rc.call(ctx, [(dev, w.t0, w.t1, w.a3, w.ok)], [ops], len(ops), 8, "self", check=False)
    finally:
        dev.close()
    assert status.tolist() == [0] and rcode == _lib.MR_ERR_STATE
    exp = rc.replica_oracle(shard, state, ops, len(ops), 8, "duration", w.t0, w.t1)
    rc.same(out[0], exp)
    assert 0 < exp.tot[:, :, 0].sum() < rc.expected("pods3", 8, "duration").tot[:, :, 0].sum()


# ---------------------------------------------------------------------------------- the Python surface
def test_windows_replicas_python(four):
    from microrank_amd.online_rca import windows_replicas

    ctx, cases, wins = four
    ops = [rc.asked(n) for n in NAMES]
    got = windows_replicas(ctx, wins, ops, m=8, what="duration")
    assert len(got) == len(cases)
    for n, a, g in zip(NAMES, ops, got):
        e = rc.expected(n, 8, "duration")
        assert list(g) == list(dict.fromkeys(a))
        for j, c in enumerate(a):
            assert g[c] == rc.as_dict(e, j), (n, c)
    got = windows_replicas(ctx, wins[:1], ops[:1])   # the defaults: m = 8, self time
    assert all(got[0][c] == rc.as_dict(rc.expected("pods3", 8, "self"), j) for j, c in enumerate(ops[0]))
    assert windows_replicas(ctx, [], []) == []


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden, regen_window

    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


def _named_oracle(adf, slo, operation_list, start, end, ops, m):
    """{op name: window_replicas' dict} by names from the DataFrame's own factorisation and the reference detector's
    lists."""
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
    asked = [pcode[o] for o in ops]
    e = rc.replica_oracle(table, state, asked, max(len(asked), 1), m, "self", int(pd.Timestamp(start).value),
                          int(pd.Timestamp(end).value))
    out = {}
    for j, key in enumerate(ops):
        d = rc.as_dict(e, j)
        d["entries"] = [(table.podop_names[x[0]],) + x[1:] for x in d["entries"]]
        out[key] = d
    return out


def test_rca_window_replicas(golden):
    from microrank_amd.online_rca import rca_window, window_replicas

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo)
    assert plain["top"]
    with_rp = rca_window(adf, start, end, slo, replicas=8)
    rp = with_rp.pop("replicas")
    assert with_rp == plain                          # every other key is what it was
    assert rp == window_replicas(adf, start, end, slo, plain["top"], m=8)
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 8)
    assert list(rp) == list(exp) and rp == exp
    assert any(r["all"] > 1 for r in rp.values()) and all(r["place"] >= 0 for r in rp.values())


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


def _expected_csv(adf, slo, operation_list, ranked, path):
    """replicas.csv as _write_replicas writes window_replicas' answer (checked against the oracle above) for the
    driver's one trigger: the data holds one 5-minute window of traffic."""
    from microrank_amd import online_rca

    start = adf["startTime"].min()
    end = start + pd.Timedelta(minutes=5)
    rows = online_rca.window_replicas(adf, start, end, slo, ranked, m=6)
    assert rows == _named_oracle(adf, slo, operation_list, start, end, ranked, 6)
    cwd = os.getcwd()
    os.makedirs(path)
    os.chdir(path)
    try:
        online_rca._write_replicas(ranked, [float(len(ranked) - i) for i in range(len(ranked))], rows)
        return open("replicas.csv", "rb").read(), rows
    finally:
        os.chdir(cwd)


def test_driver_and_stream_write_replicas_csv(golden, tmp_path, monkeypatch):
    from microrank_amd.online_rca import RCAStream

    c, adf, slo = golden
    for d in "abc":
        (tmp_path / d).mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_plain = _drive(adf, slo, c["operation_list"])
    assert os.path.exists("result.csv") and not os.path.exists("replicas.csv")   # without the keyword: no file
    monkeypatch.chdir(tmp_path / "b")
    out_rp = _drive(adf, slo, c["operation_list"], replicas=6)
    assert out_rp == out_plain
    assert open("result.csv", "rb").read() == open(tmp_path / "a" / "result.csv", "rb").read()
    assert sorted(os.listdir(".")) == ["replicas.csv", "result.csv"]
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    want, rows = _expected_csv(adf, slo, c["operation_list"], ranked, str(tmp_path / "want"))
    assert open("replicas.csv", "rb").read() == want
    table = list(csv.reader(open("replicas.csv")))
    assert table[0] == ["result", "rank", "pod", "is_result", "count_abnormal", "count_normal", "mean_abnormal",
                        "mean_normal", "max_abnormal", "max_normal", "live", "replicas"]
    assert len(table) - 1 == sum(len(rows[r]["entries"]) for r in ranked) and len(ranked) > 2
    assert sum(int(x[3]) for x in table[1:]) == len(ranked)      # each ranked op is on its own list once
    assert all((x[0] == x[2]) == (x[3] == "1") for x in table[1:])
    monkeypatch.chdir(tmp_path / "c")                            # the stream: the frame in one chunk, then close()
    with contextlib.redirect_stdout(io.StringIO()):
        s = RCAStream(slo, c["operation_list"], replicas=6)
        s.push(adf.copy())
        s.close()
    assert open("replicas.csv", "rb").read() == want
    assert sorted(os.listdir(".")) == ["replicas.csv", "result.csv"]
