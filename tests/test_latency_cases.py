"""CPU checks of the latency-evidence cases (tests/latency_cases.py): what the GPU tests rely on, said
by the numpy oracle alone -- and why self time, not duration, is the evidence."""
import numpy as np
import pytest

import latency_cases as lc


@pytest.fixture(scope="module")
def fault():
    topo, normal, abnormal = lc.fault_case()
    return (topo, abnormal) + lc.slo_and_state(normal, abnormal)


def _p50(table, state, op, what):
    out, cnt = lc.latency_oracle(table, state, lc.I64_MIN, lc.I64_MAX, [op], what, [0.5], "linear")
    assert cnt.min() > 0
    return float(out[0, 0, 0]), float(out[0, 1, 0])


def test_fault_case_partition(fault):
    topo, abnormal, a3, ok, state, t0, t1 = fault
    assert (state == 2).sum() > 0 and (state == 1).sum() > 0
    assert (state == 2).sum() + (state == 1).sum() == abnormal.n_traces
    assert lc.detector_ties(abnormal, a3, ok, t0, t1) == 0   # no float tie decides a side


def test_self_time_separates_cause_from_victims(fault):
    from microrank_amd import synth

    topo, abnormal, a3, ok, state, t0, t1 = fault
    root = int(np.unique(abnormal.podop[abnormal.meta["op"] == 0])[0])
    faulty = int(np.unique(abnormal.podop[abnormal.meta["op"] == synth.fault_op_of(topo)])[0])
    fn, fa = _p50(abnormal, state, faulty, "self")
    assert fa >= 10 * fn                       # measured 77x
    rn, ra = _p50(abnormal, state, root, "self")
    assert 0.9 <= ra / rn <= 1.1               # measured 1.002
    dn, da = _p50(abnormal, state, root, "duration")
    assert da / dn > 3                         # measured 6.7: the victim looks slow by duration


def test_dup_broken_case_has_negative_self_time():
    topo, normal, abnormal = lc.fault_case(dup=0.01, broken=0.05)
    a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
    v = lc.values(abnormal, "self")
    selected = np.isin(state[abnormal.trace], (1, 2))
    assert (v[selected] < 0).any()
    assert np.unique(abnormal.span).size < abnormal.n_spans   # a spanID code shared by two rows


def test_quiet_case_has_no_abnormal_trace():
    topo, normal, abnormal = lc.quiet_case()
    a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
    assert (state == 2).sum() == 0 and (state == 1).sum() > 0


def test_edge_table_counts():
    table, state, ops = lc.edge_table()
    assert 900 <= table.n_spans <= 1100
    out, cnt = lc.latency_oracle(table, state, lc.I64_MIN, lc.I64_MAX, ops, "self", lc.QS, "linear")
    assert set(cnt.reshape(-1).tolist()) == lc.EDGE_COUNTS
    assert cnt[0].tolist() == [0, 0] and not (table.podop == 0).any()          # an asked op with no row at all
    for o in ops[1:]:                                                          # rows of state 0 that must not count
        assert ((table.podop == o) & (state[table.trace] == 0)).any()
    assert (lc.values(table, "self") != table.duration).any()
    assert np.unique(table.span).size < table.n_spans


def test_skewed_and_banded_tables():
    table, state, sizes = lc.skewed_table()
    assert table.n_spans == 70_001 and table.n_podops == 300 and sizes[5] == 20_000
    v = lc.values(table, "self")
    assert set(v[table.podop == 7].tolist()) == {12345} and (table.podop == 7).sum() == 50
    asked = np.flatnonzero(sizes)[:63]
    assert np.isin(state[table.trace], (1, 2))[np.isin(table.podop, asked)].sum() > 4096   # the radix branch
    table, state, t0, t1 = lc.banded_table()
    inside = lc.in_window(table, t0, t1)
    assert ((table.tstart == t0) & inside).any() and ((table.tend == t1) & inside).any()
    assert ((table.tstart == t0 - 1) & (table.tend <= t1)).any() and ((table.tend == t1 + 1) & (table.tstart >= t0)).any()
