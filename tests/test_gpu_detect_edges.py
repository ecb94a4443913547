"""The window detector's routes -- mr_detect on the index (k_ix_detect) and row by row (k_win_*), the sweep
(k_ix_sweep), the detectors fused into the window builds (mr_rca_window, mr_windows_batch) -- and the
per-trace scalars of the span index they read (k_ix_trace_stats: rows, max duration, times), on
hand-built tables (detect_cases.py): traces interleaved in five row orders, verdicts that hinge on one
rounding, window bounds, detect_block's stages of 4096 entries and the sweep's integer arithmetic.
Every verdict and count is compared exactly with oracle.detect (sequential float64) and numpy row counts;
only ranking scores carry a tolerance (test_gpu_rca.test_c3_window_against_oracle's 1e-10)."""
import numpy as np
import pytest

import detect_cases as dc

pytestmark = pytest.mark.gpu
WHOLE = (dc.I64_MIN, dc.I64_MAX)


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


def _upload(ctx, table):
    from microrank_amd.preprocess_data import DeviceSpans

    return DeviceSpans(ctx, table)


# ---------------------------------------------------------------------------------- A: row order
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "per_span"])
@pytest.mark.parametrize("order", dc.ORDERS)
def test_row_order(ctx, order, uniform):
    """One logical table in five stored row orders, trace-level and per-span times: mr_detect (a window
    that holds everything, one that cuts the table), mr_detect_sweep, mr_graph_build + mr_graph_export
    (len_t = the selected traces' row counts) and the ranked window against their oracles."""
    import c_oracle
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows

    table, b = dc.order_table(order, uniform), dc.order_base()
    dev = _upload(ctx, table)
    whole, cut = dc.order_windows(table)
    for win in (whole, cut, WHOLE):
        state = dc.check_detect(ctx, dev, table, *win, b.a3, b.ok)
        lens = dc.check_graph(ctx, table, dev, state == 2)
        assert lens.tolist() == dc.trace_rows(table)[state == 2].tolist()
    if uniform:
        for sw in ((whole[0], 100, 500, 20), (whole[0] - 3, 7, 1000, 300), (0, 1000, 1000, 1)):
            dc.check_sweep(ctx, dev, table, *sw, b.a3, b.ok)
    else:
        assert dc.sweep_call(ctx, dev, 0, 7, 20, 4, b.a3, b.ok)[0] == _lib.MR_ERR_STATE
    for win in (whole, cut):
        _, na, nn, _ = dc.detect_oracle(table, *win, b.a3, b.ok)
        ref = c_oracle.rca_window(table, *win, b.a3, b.ok)
        assert (ref[2], ref[3]) == (na, nn)
        rc, codes, scores, gna, gnn = dc.rca_call(ctx, dev, *win, b.a3, b.ok)
        bc, bs, bna, bnn, _, status = rank_windows(ctx, [(dev, *win, b.a3, b.ok)])[0]
        assert rc == status == _lib.MR_OK
        assert (gna, gnn) == (int(bna), int(bnn)) == (na, nn)
        for c, s in ((codes, scores), (bc, bs)):
            assert list(c) == list(ref[0])
            np.testing.assert_allclose(s, ref[1], rtol=1e-10, atol=0)
    dev.close()


def test_append_across_cut_traces_equals_ingest(ctx):
    """mr_spans_append with a chunk boundary that cuts through traces (their kept rows first, the chunk's
    rows after other traces' rows) and a keep_from that retires traces: the appended table and
    mr_spans_ingest of the concatenation give the same code columns, the same mr_detect outputs and the
    same len_t, bit for bit -- and the oracle's."""
    import pandas as pd

    from microrank_amd.preprocess_data import SpanStream, span_table

    c1, c2, keep_from, slo = dc.append_case()
    st = SpanStream(ctx)
    st.append(c1.copy(), 0)
    table, dev = st.append(c2.copy(), keep_from)
    resident = pd.concat([c1[c1["startTime"].astype("int64") >= keep_from], c2], ignore_index=True)
    ref_table, ref_dev = span_table(resident, ctx)
    assert table.n_spans == ref_table.n_spans == len(resident) and table.n_traces == ref_table.n_traces
    assert table.trace_names == ref_table.trace_names and table.svcop_names == ref_table.svcop_names
    for a, b_ in zip(table._code_cols(), ref_table._code_cols()):
        assert np.array_equal(a, b_)
    assert all(dc.interleaving(ref_table.trace))
    a3, ok = dc.slo_by_name(ref_table, slo)
    host = dc.make_table(ref_table.trace, ref_table.svcop, ref_table.duration, ref_table.tstart, ref_table.tend,
                         podop=ref_table.podop, span=ref_table.span, parent=ref_table.parent,
                         n_traces=ref_table.n_traces, n_svcops=ref_table.n_svcops, n_podops=ref_table.n_podops)
    lo, hi = int(host.tstart.min()), int(host.tend.max())
    for win in ((lo, hi), (dc.BASE_NS + 200, dc.BASE_NS + 1200)):
        got = dc.detect_call(ctx, dev, *win, a3, ok)
        ref = dc.detect_call(ctx, ref_dev, *win, a3, ok)
        assert got[0] == ref[0] == 0 and got[1].tobytes() == ref[1].tobytes() and got[2:] == ref[2:]
        state, na, nn, rows = dc.detect_oracle(host, *win, a3, ok)
        assert got[1].tolist() == state.tolist() and got[2:] == (na, nn, rows)
        cols = (host.trace, host.podop, host.span, host.parent)
        la = dc.check_graph(ctx, table, dev, state == 2, cols)
        lb = dc.check_graph(ctx, ref_table, ref_dev, state == 2, cols)
        assert la.tobytes() == lb.tobytes()
    st.close()


# ---------------------------------------------------------------------------------- B: verdict arithmetic
@pytest.mark.parametrize("route", ["detect_uniform", "detect_per_span", "sweep", "fused"])
def test_verdict_arithmetic(ctx, route):
    """Ties (real == expect is normal, one ulp either way), sums whose association or fusing would turn
    the verdict, non-positive maxima, ops without an SLO, negative a3, 3,000 rows of one op: every trace's
    state through each route; the fused routes through the counts of each kind's window and of one
    window per trace (280 windows in one mr_windows_batch call, and one mr_rca_window call each)."""
    v = dc.verdict_case()
    table = dc.per_span(v.table) if route == "detect_per_span" else v.table
    dev = _upload(ctx, table)
    wins = [WHOLE, (int(v.table.tstart.min()), int(v.table.tend.max()))] + [v.windows[k] for k in dc.VERDICT_KINDS]
    if route.startswith("detect"):
        for win in wins:
            dc.check_detect(ctx, dev, table, *win, v.a3, v.ok)
    elif route == "sweep":   # window m = trace m's slot; then windows of 12 slots, every third slot
        t_begin = int(table.tstart.min())
        dc.check_sweep(ctx, dev, table, t_begin, 10, 4, table.n_traces + 2, v.a3, v.ok)
        dc.check_sweep(ctx, dev, table, t_begin - 5, 30, 124, 40, v.a3, v.ok)
    else:   # no entry returns the fused detectors' state: a window per trace makes its counts the state
        from microrank_amd import _lib

        dc.check_fused_counts(ctx, dev, table, wins, v.a3, v.ok)
        state = dc.detect_oracle(table, *WHOLE, v.a3, v.ok)[0]
        slots = [(10 * t - 1000, 10 * t - 996) for t in range(table.n_traces)]
        got = dc.fused_counts(ctx, dev, slots, v.a3, v.ok)
        assert got == [(_lib.MR_OK, int(s == 2), int(s == 1)) for s in state]
    dev.close()


# ---------------------------------------------------------------------------------- C: window edges
def test_window_bounds_uniform(ctx):
    """ts == t0 and te == t1 are inside, one tick further is outside; t0 == t1; an empty window returns
    MR_ERR_VALUE with n_spans_in_window == 0 and leaves the table usable."""
    from microrank_amd import _lib

    table, a3, ok, inside = dc.edge_uniform()
    dev = _upload(ctx, table)
    t0, t1 = dc.EDGE_WIN
    state = dc.check_detect(ctx, dev, table, t0, t1, a3, ok)
    assert ((state > 0) == inside).all()
    rc, _, _, _, nin = dc.detect_call(ctx, dev, 100, 200, a3, ok)
    assert (rc, nin) == (_lib.MR_ERR_VALUE, 0)
    wins = [(t0, t0), (t1, t1), (t0 + 1, t1), (t0, t1 - 1), (t0 - 1, t1 + 1), (100, 200), (t0, t1)]
    for win in wins:
        dc.check_detect(ctx, dev, table, *win, a3, ok)
    dc.check_fused_counts(ctx, dev, table, wins, a3, ok)
    for sw in ((t0, 1, t1 - t0, 3), (t0 - 1, 1, t1 - t0 + 1, 3), (t0, 35, 0, 2), (t0 - 70, 35, 35, 5)):
        dc.check_sweep(ctx, dev, table, *sw, a3, ok)
    dev.close()


def test_window_bounds_per_span(ctx):
    """Per-span times: a trace's max and op counts come from its in-window rows alone; a trace whose only
    positive duration lies outside is dropped, its inside rows counted; an empty window leaves the table
    usable."""
    from microrank_amd import _lib

    table, a3, ok, exp, rows = dc.edge_per_span()
    dev = _upload(ctx, table)
    t0, t1 = dc.EDGE_WIN
    rc, state, na, nn, nin = dc.detect_call(ctx, dev, t0, t1, a3, ok)
    assert rc == _lib.MR_OK and state.tolist() == exp.tolist() and (na, nn, nin) == (1, 2, rows)
    wins = [(500, 600), (t0, t1), (t0 - 1, t1), (t0, t1 + 1), WHOLE, (0, 5), (t0, t0), (t1, t1)]
    for win in wins:
        dc.check_detect(ctx, dev, table, *win, a3, ok)
    dc.check_fused_counts(ctx, dev, table, wins, a3, ok)
    dev.close()


def test_one_trace_one_op(ctx):
    """n_traces == 1 and n_svcops == 1 through every route."""
    table, a3, ok = dc.edge_single()
    for t in (table, dc.per_span(table)):
        dev = _upload(ctx, t)
        for win in ((4, 9), (0, 20), (5, 9), WHOLE):
            dc.check_detect(ctx, dev, t, *win, a3, ok)
        dc.check_fused_counts(ctx, dev, t, [(4, 9), (5, 9), (0, 20)], a3, ok)
        if t is table:
            for sw in ((4, 1, 5, 1), (0, 2, 5, 6), (3, 1, 4, 3)):
                dc.check_sweep(ctx, dev, t, *sw, a3, ok)
        dev.close()


# ---------------------------------------------------------------------------------- D: detect_block staging
@pytest.mark.parametrize("name", list(dc.STAGE_TABLES))
def test_detect_block_stages(ctx, name, monkeypatch):
    """First blocks of 4095, 4096, 4097 and 8193 (trace, service-op) entries, a trace across the stage edge,
    a trace of 4,100 service-ops, blocks of one-entry traces, 1 / 255 / 256 / 257 / 513 traces; every
    trace's expect is its real or one ulp below, so a term added out of order turns verdicts.  mr_detect
    (index and row-level) and mr_detect_sweep in full, the fused routes -- the layout-order build where the
    table allows it, and the index build's fused detector -- by counts."""
    s = dc.stage_case(name)
    table = s.table
    dev = _upload(ctx, table)
    lo, hi = int(table.tstart.min()), int(table.tend.max())
    mid = (lo + hi) // 2
    wins = [WHOLE, (lo, hi), (lo, mid), (mid - 40, hi)]
    state = dc.check_detect(ctx, dev, table, *WHOLE, s.a3, s.ok)
    assert state.tolist() == s.state.tolist()
    for win in wins[1:]:
        dc.check_detect(ctx, dev, table, *win, s.a3, s.ok)
    dc.check_sweep(ctx, dev, table, lo, 5, 4, table.n_traces + 1, s.a3, s.ok)
    dc.check_sweep(ctx, dev, table, lo - 2, 640, 1400, 5, s.a3, s.ok)
    dc.check_fused_counts(ctx, dev, table, wins, s.a3, s.ok)
    monkeypatch.setenv("MR_NO_LO_WIN", "1")   # (read per call: the index build with the fused detector)
    dc.check_fused_counts(ctx, dev, table, wins, s.a3, s.ok)
    monkeypatch.delenv("MR_NO_LO_WIN")
    dev.close()
    rows = dc.per_span(table)
    dev = _upload(ctx, rows)
    for win in wins[:3]:
        dc.check_detect(ctx, dev, rows, *win, s.a3, s.ok)
    dev.close()


# ---------------------------------------------------------------------------------- E: sweep arithmetic
@pytest.mark.parametrize("sweep", dc.SWEEPS, ids=lambda s: "b{}_g{}_w{}_n{}".format(*s))
def test_sweep_arithmetic(ctx, sweep):
    """Window starts before and after traces, a grain that does not divide the window, window = 0, traces
    longer than the window and past the last window, 0 / 1 / 4096 / 4097 windows (the two sides of the LDS
    histogram)."""
    table, a3, ok = dc.sweep_table()
    dev = _upload(ctx, table)
    dc.check_sweep(ctx, dev, table, *sweep, a3, ok)
    dev.close()


def test_sweep_row_counters_around_65536(ctx):
    """Traces of 65,536 and 65,537 rows: the two sides of the sweep's switch from 32-bit block partials to
    64-bit row counters; n_rows as int64.  mr_detect and the fused routes count the same rows."""
    table, a3, ok = dc.sweep_big_table()
    dev = _upload(ctx, table)
    for sw in dc.BIG_SWEEPS:
        dc.check_sweep(ctx, dev, table, *sw, a3, ok)
    wins = [(0, 9), (10, 19), (0, 19)]
    for win in wins:
        dc.check_detect(ctx, dev, table, *win, a3, ok)
    dc.check_fused_counts(ctx, dev, table, wins, a3, ok)
    dev.close()
