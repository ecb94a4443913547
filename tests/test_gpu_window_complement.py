"""The complement form of the layout-order window build against its direct form.

A window's graph of normal traces is the table's totals minus the graph of abnormal traces minus
the traces in neither graph (mr_internal.h, mr_spans.lo_cmp_ok); MR_LO_COMPLEMENT=1 forces that
form wherever the table carries its data, 0 the direct form, unset chooses by the table's time
summary.  Both forms must give the same words, so everything here is compared exactly: statuses,
abnormal and normal counts, edges and top codes equal, scores byte for byte.

Tables of 40 ops / 3000 traces: more than the 1024 traces of one build block, so several blocks
and several partial rows.  The detector thresholds are one constant per table: with a3 = c for
every service-op a trace is abnormal when (max duration / 1000) / spans > c, so a quantile of that
ratio over the traces fixes the abnormal share."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import detect_cases as dc

pytestmark = pytest.mark.gpu
FORMS = ("1", "0")   # MR_LO_COMPLEMENT: complement, direct


def _counts():
    from microrank_amd import _lib

    a, b = C.c_int64(), C.c_int64()
    assert _lib.load().mr_lo_complement_counts(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _a3(table, q=None, c=None):
    """One threshold for every service-op: the q-quantile of the traces' (max duration / 1000) / spans
    (a share 1 - q of the traces is abnormal), or the constant c."""
    if c is None:
        n = np.bincount(table.trace, minlength=table.n_traces).astype(np.float64)
        mx = np.zeros(table.n_traces)
        np.maximum.at(mx, table.trace, table.duration.astype(np.float64))
        c = float(np.quantile((mx / 1000.0 / np.maximum(n, 1))[n > 0], q))
    return np.full(table.n_svcops, c, np.float64), np.ones(table.n_svcops, np.uint8)


def _same(a, b, what):
    assert a[5] == b[5], what
    assert a[2:] == b[2:], what
    assert list(a[0]) == list(b[0]), what
    assert a[1].tobytes() == b[1].tobytes(), what


def _rank(ctx, wins, monkeypatch, form, chunk=None):
    from microrank_amd.online_rca import rank_windows

    for k, v in (("MR_LO_COMPLEMENT", form), ("MR_WIN_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    return rank_windows(ctx, wins)


def _rca(ctx, table, dev, t0, t1, a3, monkeypatch, form):
    from microrank_amd.online_rca import rca_window

    monkeypatch.setenv("MR_LO_COMPLEMENT", form)
    slo = {name: (float(a3[i]), 0.0) for i, name in enumerate(table.svcop_names)}
    return rca_window(None, int(t0), int(t1), slo, ctx=ctx, table=table, dev=dev)


@pytest.fixture(scope="module")
def tables():
    """(SpanTable, DeviceSpans) per name: two 40-op / 3000-trace tables, one trace of the first, a
    12-trace table (fewer than 16 traces per op)."""
    from microrank_amd import _lib, synth
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    out = {}
    for name, (nt, seed) in {"a": (3000, 11), "b": (3000, 12), "few": (12, 13)}.items():
        _, _, ab = synth.window_pair(40, nt, seed)
        out[name] = ab
    a = out["a"]
    one = a.take(np.flatnonzero(a.trace == a.trace[0]))
    one.trace, one.trace_names = np.zeros(one.n_spans, np.int32), [a.trace_names[int(a.trace[0])]]
    out["one"] = one
    devs = {k: DeviceSpans(ctx, v) for k, v in out.items()}
    yield {k: (out[k], devs[k]) for k in out}
    for d in devs.values():
        d.close()


def _windows(tables):
    """The windows of the issue's list over the synthetic tables: (name, (dev, t0, t1, a3, ok))."""
    wins = []
    for key in ("a", "b"):
        tab, dev = tables[key]
        lo, hi = int(tab.tstart.min()), int(tab.tend.max())
        a3, ok = _a3(tab, q=0.9)
        wins.append((f"{key}: whole table", (dev, lo, hi, a3, ok)))
        wins.append((f"{key}: half the table", (dev, lo, lo + (hi - lo) // 2, a3, ok)))
    tab, dev = tables["a"]
    lo, hi = int(tab.tstart.min()), int(tab.tend.max())
    wins.append(("a: every trace abnormal", (dev, lo, hi) + _a3(tab, c=1e-12)))
    wins.append(("a: no trace abnormal", (dev, lo, hi) + _a3(tab, c=1e12)))
    wins.append(("a: empty window", (dev, 0, 1) + _a3(tab, q=0.9)))
    tab, dev = tables["one"]
    wins.append(("one trace", (dev, int(tab.tstart.min()), int(tab.tend.max())) + _a3(tab, c=1e-12)))
    tab, dev = tables["few"]
    wins.append(("fewer than 16 traces per op", (dev, int(tab.tstart.min()), int(tab.tend.max())) + _a3(tab, q=0.5)))
    return wins


@pytest.mark.parametrize("chunk", ["1", "4"])
def test_rank_windows_complement_equals_direct(tables, monkeypatch, chunk):
    """rank_windows over every window of the list in one call, in chunks of 1 and of 4 (windows of
    both tables and of several shapes share a launch): forced complement against forced direct."""
    from microrank_amd import _lib

    ctx = _lib.default_context()
    wins = _windows(tables)
    c0 = _counts()
    got = {f: _rank(ctx, [w for _, w in wins], monkeypatch, f, chunk) for f in FORMS}
    c1 = _counts()
    assert c1[0] - c0[0] == len(wins) and c1[1] == c0[1]   # every window took the form once; no rebuild
    for (name, _), a, b in zip(wins, got["1"], got["0"]):
        _same(a, b, name)
    by = {name: r for (name, _), r in zip(wins, got["1"])}
    assert by["a: whole table"][5] == 0 and by["a: whole table"][2] > 0 and by["a: whole table"][3] > 0
    assert len(by["a: whole table"][0]) == 11 and by["a: half the table"][2] > 0
    assert by["a: every trace abnormal"][3] == 0 and by["a: no trace abnormal"][2] == 0
    assert by["a: empty window"][5] == _lib.MR_ERR_VALUE
    assert by["fewer than 16 traces per op"][2] > 0 and by["fewer than 16 traces per op"][3] > 0


def test_automatic_form_by_the_time_summary(tables, monkeypatch):
    """MR_LO_COMPLEMENT unset: the window over the whole table takes the complement form, the one
    over half of it the direct form (the summary bounds the traces left out above a quarter), and
    both rank as the forced forms do."""
    from microrank_amd import _lib

    ctx = _lib.default_context()
    wins = dict(_windows(tables))
    for name, n_cmp in (("a: whole table", 1), ("a: half the table", 0)):
        c0 = _counts()
        auto = _rank(ctx, [wins[name]], monkeypatch, None)[0]
        assert _counts()[0] - c0[0] == n_cmp, name
        for f in FORMS:
            _same(auto, _rank(ctx, [wins[name]], monkeypatch, f)[0], name)


def test_rca_window_complement_equals_direct(tables, monkeypatch):
    from microrank_amd import _lib

    ctx = _lib.default_context()
    tab, dev = tables["b"]
    lo, hi = int(tab.tstart.min()), int(tab.tend.max())
    a3, _ = _a3(tab, q=0.9)
    for t1 in (hi, lo + (hi - lo) // 2):
        c0 = _counts()
        a, b = (_rca(ctx, tab, dev, lo, t1, a3, monkeypatch, f) for f in FORMS)
        assert _counts()[0] - c0[0] == 1
        assert a["n_abnormal"] > 0 and a["n_normal"] > 0 and len(a["top"]) == 11
        assert a["top"] == b["top"] and (a["n_abnormal"], a["n_normal"], a["edges"]) == \
            (b["n_abnormal"], b["n_normal"], b["edges"])
        assert np.asarray(a["score"]).tobytes() == np.asarray(b["score"]).tobytes()


def test_complement_index_failure_keeps_direct_form(tables, monkeypatch):
    """The complement data is a best-effort part of the index: a failure inside it
    (MR_LO_CMP_TEST_FAIL, read per table) leaves the upload successful, the error text clear and
    the table on the direct form even where the complement form is asked for."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    tab, good = tables["a"]
    monkeypatch.setenv("MR_LO_CMP_TEST_FAIL", "1")
    bad = DeviceSpans(ctx, tab)
    monkeypatch.delenv("MR_LO_CMP_TEST_FAIL")
    assert (_lib.load().mr_last_error(ctx.h) or b"") == b""
    w = (int(tab.tstart.min()), int(tab.tend.max())) + _a3(tab, q=0.9)
    c0 = _counts()
    b = _rank(ctx, [(bad,) + w], monkeypatch, "1")[0]
    assert _counts()[0] == c0[0]
    _same(_rank(ctx, [(good,) + w], monkeypatch, "1")[0], b, "table without the complement data")
    bad.close()


# ------------------------------------------------------------------ hand-built: first-row candidates
# 200 traces; op 0 once in every trace; op 1 once in the traces 0..127 (X_ALL) or 0..15 (X_EARLY).
# Rows: op 1 of the traces 0..15 (rows 0..15), op 0 of every trace (rows 16..215), op 1 of the traces
# 16..127 (rows 216..327).  The traces 0..15 are abnormal by their durations, every other one normal.
# With op 1 in 128 traces of 328 rows its candidate threshold is 328 * 64 / 128 + 1 = 165: its
# candidates are exactly its 16 earliest traces, all abnormal, while the 17th (and 111 more) is normal.
def _hand_table(x_traces):
    early = np.arange(16)
    late = np.arange(16, x_traces)
    trace = np.concatenate([early, np.arange(200), late])
    op = np.concatenate([np.ones(16, np.int64), np.zeros(200, np.int64), np.ones(late.size, np.int64)])
    dur = np.where(trace < 16, 1_000_000, 1_000)       # µs: 1000 ms against 1 ms
    ts = 100 + trace
    return dc.make_table(trace, op, dur, ts, ts + 10, podop=op, n_traces=200, n_svcops=2, n_podops=2)


@pytest.mark.parametrize("chunk", ["1", "4"])
def test_candidates_exhausted_rebuilds_directly(monkeypatch, chunk):
    """Op 1's 16 earliest traces are abnormal and its 17th is normal: graph 1 holds op 1 but none of
    its candidates, so the window is flagged, rebuilt in the direct form and ranks as the direct
    form does.  The same table with op 1 in the 16 abnormal traces only: op 1 is absent from
    graph 1 and nothing is rebuilt."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    a3, ok = np.full(2, 10.0), np.ones(2, np.uint8)   # expect = 10 ms per span
    for x_traces, rebuilt in ((128, 1), (16, 0)):
        dev = DeviceSpans(ctx, _hand_table(x_traces))
        wins = [(dev, 0, 1000, a3, ok)] * 2 + [(dev, 0, 1, a3, ok)]
        c0 = _counts()
        a = _rank(ctx, wins, monkeypatch, "1", chunk)
        c1 = _counts()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (3, 2 * rebuilt)
        b = _rank(ctx, wins, monkeypatch, "0", chunk)
        assert _counts() == c1
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (x_traces, i))
        assert a[0][5] == 0 and (a[0][2], a[0][3]) == (16, 184) and a[2][5] == _lib.MR_ERR_VALUE
        assert sorted(a[0][0].tolist()) == [0, 1]
        dev.close()


# The other two threshold tiers.  1200 traces, 2500 rows: op 0 once in every trace (rows 0..1199), then
# op 1 in the traces 0..199 (rows 1200..1399), then op 2 in the traces 0..1099 (rows 1400..2499).
#   op 1: 200 entries, r1 = 2500 * 64 / 200 + 1 = 801: none below it, all 200 below 8 r1 -- the second tier;
#   op 2: 1100 entries, r1 = 146, 8 r1 = 1168: none below either -- every row (1100 candidates);
#   op 0: 1200 entries, r1 = 134: 134 below it -- the first tier.
# The traces 0..n_abnormal-1 are abnormal.  With 10 of them every op's 11th candidate is normal; with 300
# op 2's first LO_CMP_SCAN = 256 candidates are all abnormal while graph 1 holds the op: rebuilt directly.
# The third case has 2400 traces and op 2 in 2300 of them (4900 rows; r1 = 137, 8 r1 = 1096, its first row
# 2600): a segment of 2300 candidates, past the 2048 that the per-op sort of the index takes in LDS.
def _late_table(n_abnormal, nt, n2):
    trace = np.concatenate([np.arange(nt), np.arange(200), np.arange(n2)])
    op = np.concatenate([np.zeros(nt, np.int64), np.ones(200, np.int64), np.full(n2, 2, np.int64)])
    dur = np.where(trace < n_abnormal, 1_000_000, 1_000)
    ts = 100 + trace
    return dc.make_table(trace, op, dur, ts, ts + 10, podop=op, n_traces=nt, n_svcops=3, n_podops=3)


@pytest.mark.parametrize("n_abnormal,rebuilt,nt,n2", [(10, 0, 1200, 1100), (300, 1, 1200, 1100), (10, 0, 2400, 2300)])
def test_late_first_rows_take_the_wider_thresholds(monkeypatch, n_abnormal, rebuilt, nt, n2):
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    a3, ok = np.full(3, 10.0), np.ones(3, np.uint8)
    dev = DeviceSpans(ctx, _late_table(n_abnormal, nt, n2))
    wins = [(dev, 0, 10_000, a3, ok)]
    c0 = _counts()
    a = _rank(ctx, wins, monkeypatch, "1")[0]
    c1 = _counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, rebuilt)
    b = _rank(ctx, wins, monkeypatch, "0")[0]
    _same(a, b, n_abnormal)
    assert a[5] == 0 and (a[2], a[3]) == (n_abnormal, nt - n_abnormal) and sorted(a[0].tolist()) == [0, 1, 2]
    dev.close()


def test_appended_table_ranks_as_fresh_upload(monkeypatch):
    """A table grown by mr_spans_append (its index, totals and candidates rebuilt by every append)
    ranks after each append as a fresh upload of the same rows, in both forms."""
    from microrank_amd import _lib, synth
    from microrank_amd.preprocess_data import SpanStream, span_table

    _, adf = synth.stream_dataframes(24, 1200, 5, minutes=30.0)
    ctx = _lib.default_context()
    t0 = adf["startTime"].min()
    bucket = ((adf["startTime"] - t0) // pd.Timedelta(minutes=8)).to_numpy()
    cuts = [t0 + pd.Timedelta(minutes=m) for m in (0, 0, 9, 9)]
    st = SpanStream(ctx)
    resident, ranked = None, 0
    for i, bk in enumerate(np.unique(bucket)):
        chunk = adf[bucket == bk].copy()
        cut = cuts[min(i, len(cuts) - 1)]
        table, dev = st.append(chunk, int(cut.value))
        if resident is not None:
            resident = resident[resident["startTime"] >= cut]
        resident = (chunk if resident is None else pd.concat([resident, chunk], ignore_index=True)).reset_index(drop=True)
        ref_table, ref_dev = span_table(resident.copy(), ctx)
        assert table.svcop_names == ref_table.svcop_names
        g = resident.groupby("traceID")["duration"]
        c = float(np.quantile((g.max() / 1000.0 / g.size()).to_numpy(), 0.8))
        w = (int(resident["startTime"].min().value), int(resident["endTime"].max().value),
             np.full(table.n_svcops, c), np.ones(table.n_svcops, np.uint8))
        c0 = _counts()
        got = [_rank(ctx, [(d,) + w], monkeypatch, f)[0] for d in (dev, ref_dev) for f in FORMS]
        assert _counts()[0] - c0[0] == 2
        for r in got[1:]:
            _same(got[0], r, f"append {i}")
        ranked += got[0][5] == 0 and got[0][2] > 0 and got[0][3] > 0
    assert ranked >= 2
    st.close()
