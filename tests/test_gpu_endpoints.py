"""GPU checks of mr_spans_entry_ops and mr_windows_endpoints (csrc/mr_endpoints.hip): every trace's entry operation,
and per asked slot the window's traces grouped by it -- the count, the summed and the largest trace duration on each
side of the window's detector partition, the first m endpoints under the order, the live count and the totals.
Every comparison is exact integer equality of all seven outputs with the numpy oracle of tests/endpoint_cases.py
(the span table's rows and oracle.detect's partition); no tolerance anywhere."""
import contextlib
import csv
import ctypes as C
import io
import os

import numpy as np
import pandas as pd
import pytest

import detect_cases as dc
import endpoint_cases as ec
import kind_breakdown_cases as kb
import latency_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


@pytest.fixture(scope="module")
def dev_of(ctx):
    """case -> its DeviceSpans, uploaded once per module."""
    from microrank_amd.preprocess_data import DeviceSpans

    devs = {}

    def get(w):
        if w.name not in devs:
            devs[w.name] = DeviceSpans(ctx, w.table)
        return devs[w.name]

    yield get
    for d in devs.values():
        d.close()


def _check(ctx, dev, w, ops, m, k=None, windows=None):
    """One call over `windows` (default: the case's own) of one table, every window asked `ops`: each equals the oracle."""
    from microrank_amd import _lib

    windows = [(w.t0, w.t1)] if windows is None else windows
    k = k or max(len(ops), 1)
    _, out, status = ec.call(ctx, [ec.win_of(dev, w, a, b) for a, b in windows], [ops] * len(windows), k, m)
    for (a, b), o, st in zip(windows, out, status.tolist()):
        state = w.state if (a, b) == (w.t0, w.t1) else ec.state_of(w.table, a, b)
        assert st == (_lib.MR_OK if state is not None else _lib.MR_ERR_VALUE), (a, b)
        ec.same(o, ec.endpoint_oracle(w.table, state, ops, k, m))
    return out


# ---------------------------------------------------------------------------------- the index
def test_entry_ops_rules(ctx, dev_of):
    w = ec.index()
    assert dev_of(w).entry_ops().tolist() == ec.IX_EXPECT
    assert dev_of(w).entry_ops().tolist() == ec.IX_EXPECT            # kept with the table: the second call reads it
    assert dev_of(ec.one_row()).entry_ops().tolist() == [0]
    for w in (ec.distinct(), ec.ranked(), ec.wide(), ec.wrapping(), ec.cut(ec.TILE + 1)):
        got = dev_of(w).entry_ops()
        assert got.dtype == np.int32 and got.tolist() == ec.entry_ops(w.table).tolist(), w.name


@pytest.mark.parametrize("name", dc.ORDERS)
def test_entry_ops_interleaved_orders(ctx, dev_of, name):
    w = ec.order_table(name)
    assert dev_of(w).entry_ops().tolist() == ec.entry_ops(w.table).tolist()
    _check(ctx, dev_of(w), w, [-1, 0, 7, 17], 8, windows=[(w.t0, w.t1), dc.ORDER_CUT])


def test_entry_ops_unknown_parent_id(ctx):
    """Through the string ingest: a ParentSpanId that is no spanID of the table makes a root row."""
    from microrank_amd.preprocess_data import span_table

    table, dev = span_table(ec.unknown_parent_frame(), ctx)
    assert [table.podop_names[c] for c in dev.entry_ops()] == ["p_x", "p_y"]


# ---------------------------------------------------------------------------------- counts, sums, order
def test_distinct_traces(ctx, dev_of):
    w = ec.distinct()
    out = _check(ctx, dev_of(w), w, [ec.X_D, ec.E_D, -1, ec.Y_D], 4)
    assert out[0].cnt[0, 0].tolist() == [1, 2]                       # 3 traces hold X_D's 73 spans
    assert out[0].cnt[1, 0].tolist() == [2, 2] and out[0].op[:, 0].tolist() == [ec.E_D] * 4


def test_sums_wrap(ctx, dev_of):
    w = ec.wrapping()
    out = _check(ctx, dev_of(w), w, [-1, 2], 2)
    assert out[0].sum[0, 0].tolist() == [-(1 << 63), 4] and out[0].max[1, 0].tolist() == [-(1 << 63), 4]


@pytest.mark.parametrize("m", [1, 4, 5, 6, 32])
def test_order_and_m(ctx, dev_of, m):
    w = ec.ranked()
    out = _check(ctx, dev_of(w), w, [-1, ec.X_R, ec.GONE_R, 4, -1], m)
    assert out[0].op[0, :min(m, 5)].tolist() == [4, 1, 2, ec.NONE, 3][:m]
    assert out[0].live.tolist() == [5, 5, 0, 1, 5] and out[0].n.tolist() == [min(m, x) for x in (5, 5, 0, 1, 5)]


# ---------------------------------------------------------------------------------- table paths
def test_direct_and_hashed_tables(ctx, dev_of):
    w = ec.ranked()
    _check(ctx, dev_of(w), w, [ec.X_R], 8)                            # one slot, 5 keys a side: direct-mapped
    w = ec.wide()
    for m in ec.MS:
        _check(ctx, dev_of(w), w, [ec.X_W], m)                        # one slot over 601 keys a side: hashed
    out = _check(ctx, dev_of(w), w, ec.wide_asked(), 32)              # 64 asked ops, duplicates, -1 in the middle
    assert out[0].live[0] == ec.N_WIDE and out[0].live[32] == ec.N_WIDE   # (X_W and -1: every trace, every endpoint)
    assert out[0].op[4].tolist() == out[0].op[1].tolist() and out[0].n[4] > 0   # a duplicate is answered each time


# ---------------------------------------------------------------------------------- windows
def test_windows_of_one_table(ctx, dev_of):
    from microrank_amd import _lib

    w = ec.ranked()
    wins = ec.ranked_windows()
    ops = [-1, ec.X_R, 1, ec.GONE_R]
    out = _check(ctx, dev_of(w), w, ops, 8, windows=wins)             # an empty window between two live ones
    assert out[2].op.tolist() == [[-1] * 8] * 4 and not out[2].cnt.any() and not out[2].tot.any()
    assert out[1].tot[0, :, 0].sum() < out[0].tot[0, :, 0].sum()      # the half window leaves traces out
    alone = [ec.call(ctx, [ec.win_of(dev_of(w), w, a, b)], [ops], 4, 8)[1][0] for a, b in wins]
    assert ec.raw_bytes(alone) == ec.raw_bytes(out)                   # a window's place and neighbours do not matter
    _, rev, st = ec.call(ctx, [ec.win_of(dev_of(w), w, a, b) for a, b in wins[::-1]], [ops] * 4, 4, 8)
    assert ec.raw_bytes(rev[::-1]) == ec.raw_bytes(out) and st.tolist() == [0, _lib.MR_ERR_VALUE, 0, 0]
    # n_ops = 0 beside an asked window, and in a call of its own
    _, o, st = ec.call(ctx, [ec.win_of(dev_of(w), w)] * 2, [[], ops], 4, 8)
    assert st.tolist() == [0, 0]
    ec.same(o[0], ec.endpoint_oracle(w.table, w.state, [], 4, 8))
    ec.same(o[1], ec.endpoint_oracle(w.table, w.state, ops, 4, 8))
    _, o, st = ec.call(ctx, [ec.win_of(dev_of(w), w)], [[]], 4, 8)
    ec.same(o[0], ec.endpoint_oracle(w.table, w.state, [], 4, 8))
    assert st.tolist() == [0]


def test_tables_of_one_call(ctx, dev_of):
    cases = [ec.ranked(), ec.wide(), ec.distinct(), ec.one_row()]
    ops = [[-1, ec.X_R], [ec.X_W, -1, 5], [ec.X_D], [0, -1]]
    _, out, st = ec.call(ctx, [ec.win_of(dev_of(w), w) for w in cases], ops, 3, 8)
    assert st.tolist() == [0] * 4
    for w, a, o in zip(cases, ops, out):
        ec.same(o, ec.endpoint_oracle(w.table, w.state, a, 3, 8))


# ---------------------------------------------------------------------------------- cuts
@pytest.mark.parametrize("n", [ec.TILE - 1, ec.TILE, ec.TILE + 1])
def test_tile_edges(ctx, dev_of, n):
    w = ec.cut(n)
    _check(ctx, dev_of(w), w, [-1, 0, 3, 6], 8)


def test_invariance_under_chunks_and_blocks(ctx, dev_of, monkeypatch):
    cases = [ec.wide(), ec.ranked(), ec.wide(), ec.cut(ec.TILE + 1)]
    ops = [ec.wide_asked()[:40], [-1, ec.X_R], [ec.X_W], [-1, 2]]
    wins = [ec.win_of(dev_of(w), w) for w in cases]
    _, out, status = ec.call(ctx, wins, ops, 40, 8)
    ref = ec.raw_bytes(out)
    for w, a, o in zip(cases, ops, out):
        ec.same(o, ec.endpoint_oracle(w.table, w.state, a, 40, 8))
    for chunk in (None, "1"):
        for blocks in (None, "1", "3"):
            for name, v in (("MR_EP_CHUNK", chunk), ("MR_EP_BLOCKS", blocks)):   # (both read per call)
                monkeypatch.delenv(name, raising=False) if v is None else monkeypatch.setenv(name, v)
            _, o, s = ec.call(ctx, wins, ops, 40, 8)
            assert ec.raw_bytes(o) == ref and s.tolist() == status.tolist(), (chunk, blocks)


# ---------------------------------------------------------------------------------- refusals
def test_errors_leave_the_context_usable(ctx, dev_of):
    import dataclasses

    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    w = ec.ranked()
    ops = [-1, ec.X_R]
    win = ec.win_of(dev_of(w), w)

    def good():
        _, out, status = ec.call(ctx, [win], [ops], 2, 8)
        assert status.tolist() == [0]
        ec.same(out[0], ec.endpoint_oracle(w.table, w.state, ops, 2, 8))

    good()
    for bad in (dict(k=0), dict(k=65), dict(m=0), dict(m=33), dict(ops=[[0, 1, 2]]), dict(ops=[[w.table.n_podops]]),
                dict(ops=[[-2]])):
        kw = dict(ops=[ops], k=2, m=8)
        kw.update(bad)
        rcode, _, _ = ec.call(ctx, [win], kw["ops"], kw["k"], kw["m"], check=False)
        assert rcode == _lib.MR_ERR_ARG, bad
        good()
    n1 = np.zeros(1, np.int32)   # a null pointer
    rcode = _lib.load().mr_windows_endpoints(ctx.h, 1, None, None, None, None, None, None, _lib.ptr(n1, C.c_int32), 1, 1,
                                             None, None, None, None, None, None, None, None)
    assert rcode == _lib.MR_ERR_ARG
    assert _lib.load().mr_spans_entry_ops(ctx.h, dev_of(w).h, None) == _lib.MR_ERR_ARG
    good()
    # MR_ERR_STATE; the message names the case
    shard = w.table.shard(0, 2)
    assert shard.row is not None and 0 < shard.n_spans < w.table.n_spans
    timeless = dataclasses.replace(w.table, tstart=None, tend=None)
    per_span = dc.per_span(dc.order_table("grouped", True))
    for table, window, words in ((shard, (w.t0, w.t1), ["trace shard"]),
                                 (timeless, ec.WHOLE, ["trace-level times"]),
                                 (per_span, ec.WHOLE, ["trace-level times"])):
        dev = DeviceSpans(ctx, table)
        try:
            a3, ok = ec.slo(table)
            rcode, _, _ = ec.call(ctx, [(dev, window[0], window[1], a3, ok)], [[-1]], 1, 8, check=False)
            assert rcode == _lib.MR_ERR_STATE, words
            for word in words:
                assert word in lc.last_error(ctx), word
            if table is shard:
                ep = np.zeros(table.n_traces, np.int32)
                assert _lib.load().mr_spans_entry_ops(ctx.h, dev.h, _lib.ptr(ep, C.c_int32)) == _lib.MR_ERR_STATE
                assert "trace shard" in lc.last_error(ctx)
        finally:
            dev.close()
        good()


# ---------------------------------------------------------------------------------- the Python surface
def test_windows_endpoints_python(ctx, dev_of):
    from microrank_amd.online_rca import windows_endpoints

    cases = [ec.ranked(), ec.distinct()]
    ops = [[None, ec.X_R, ec.GONE_R, ec.X_R], [ec.X_D, None]]
    wins = [ec.win_of(dev_of(w), w) for w in cases]
    got = windows_endpoints(ctx, wins, ops, m=4)
    for w, a, g in zip(cases, ops, got):
        codes = [-1 if c is None else c for c in a]
        e = ec.endpoint_oracle(w.table, w.state, codes, len(codes), 4)
        assert list(g) == list(dict.fromkeys(a))
        for j, c in enumerate(a):
            assert g[c] == ec.as_dict(e, j), (w.name, c)
    assert got[0][None]["entries"][3][0] is None                     # MR_EP_NONE is None in Python
    got = windows_endpoints(ctx, wins[:1], ops[:1])                  # the default: m = 8
    e = ec.endpoint_oracle(cases[0].table, cases[0].state, [-1], 1, 8)
    assert got[0][None] == ec.as_dict(e, 0)
    assert windows_endpoints(ctx, [], []) == []


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden, regen_window

    c = load_golden("pods_dup_broken.json")
    _, adf = regen_window(c)
    slo = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in c["slo"].items()}
    return c, adf, slo


def _named_oracle(adf, slo, operation_list, start, end, ops, m):
    """{None or op name: window_endpoints' dict} by names from the DataFrame's own factorisation and the reference
    detector's lists."""
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
    e = ec.endpoint_oracle(table, state, asked, len(asked), m)
    out = {}
    for j, key in enumerate([None] + list(ops)):
        d = ec.as_dict(e, j)
        d["entries"] = [((table.podop_names[x[0]] if x[0] is not None else None),) + x[1:] for x in d["entries"]]
        out[key] = d
    return out


def test_rca_window_endpoints(golden):
    from microrank_amd.online_rca import rca_window, window_endpoints

    c, adf, slo = golden
    start, end = pd.Timestamp(c["detect"]["start_ns"]), pd.Timestamp(c["detect"]["end_ns"])
    plain = rca_window(adf, start, end, slo)
    assert plain["top"]
    with_ep = rca_window(adf, start, end, slo, kind_breakdown=4, kind_by="endpoint")
    got = with_ep.pop("endpoints")
    assert with_ep == plain                          # every other key is what it was; no "kinds"
    assert got == window_endpoints(adf, start, end, slo, plain["top"], m=4)
    exp = _named_oracle(adf, slo, c["operation_list"], start, end, plain["top"], 4)
    assert list(got) == list(exp) and got == exp
    assert got[None]["live"] >= 1 and sum(got[None]["total"][:2]) == plain["n_abnormal"] + plain["n_normal"]
    with_kinds = rca_window(adf, start, end, slo, kind_breakdown=4)   # the keyword alone: the trace kinds, as before
    assert "kinds" in with_kinds and "endpoints" not in with_kinds


def _drive(df, slo, ops, **kw):
    from microrank_amd import online_rca

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        online_rca.online_anomaly_detect_RCA(df.copy(), slo, ops, **kw)
    return buf.getvalue()


def test_driver_writes_endpoints_csv(golden, tmp_path, monkeypatch):
    from microrank_amd import online_rca

    c, adf, slo = golden
    for d in "ab":
        (tmp_path / d).mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out_plain = _drive(adf, slo, c["operation_list"])
    assert os.listdir(".") == ["result.csv"]
    monkeypatch.chdir(tmp_path / "b")
    assert _drive(adf, slo, c["operation_list"], kind_breakdown=6, kind_by="endpoint") == out_plain
    assert open("result.csv", "rb").read() == open(tmp_path / "a" / "result.csv", "rb").read()
    assert sorted(os.listdir(".")) == ["endpoints.csv", "result.csv"]          # kinds.csv is not written
    ranked = [r["result"] for r in csv.DictReader(open("result.csv"))]
    start = adf["startTime"].min()                   # the driver's one trigger: the data holds one 5-minute window
    rows = _named_oracle(adf, slo, c["operation_list"], start, start + pd.Timedelta(minutes=5), ranked, 6)
    got = open("endpoints.csv", "rb").read()
    (tmp_path / "want").mkdir()
    monkeypatch.chdir(tmp_path / "want")
    online_rca._write_endpoints(ranked, [float(len(ranked) - i) for i in range(len(ranked))], rows)
    assert got == open("endpoints.csv", "rb").read()
    table = list(csv.reader(io.StringIO(got.decode())))
    assert table[0] == ["result", "rank", "endpoint", "traces_abnormal", "traces_normal", "mean_abnormal", "mean_normal",
                        "max_abnormal", "max_normal", "live"]
    assert table[1][:2] == ["*", "0"] and len(table) - 1 == sum(len(r["entries"]) for r in rows.values()) and len(ranked) > 2
