"""CPU checks of the kind-breakdown cases (tests/kind_breakdown_cases.py): the shapes that make the GPU
cases of tests/test_gpu_kind_breakdown.py meaningful, on the numpy oracle alone (no GPU needed)."""
import numpy as np

import kind_breakdown_cases as kb


def test_ties_has_large_kinds_on_both_sides():
    s = kb.summary(kb.window("ties"))
    assert (s.traces, s.live, s.multi, s.both, s.largest) == (2000, 254, 136, 33, 407)
    assert s.pairs[:3] == [(64, 5), (62, 0), (52, 82)]


def test_mid_is_mostly_singleton_kinds():
    s = kb.summary(kb.window("mid"))
    assert (s.traces, s.live) == (1000, 792)


def test_ragged_ties_inside_the_top_and_pads():
    w = kb.window("ragged")
    s = kb.summary(w)
    assert s.pairs[:2] == [(2, 0), (2, 0)]            # two kinds tie: the smaller rep decides
    e = kb.expected("ragged", 32)
    assert ((e.n > 0) & (e.n < 32)).any()             # slots whose selected kinds number fewer than m
    assert e.kinds[kb.asked_ops(w).index(-1)] == s.live


def test_one_trace_has_one_abnormal_trace():
    w = kb.window("one_trace")
    assert int((w.state == 2).sum()) == 1
    e = kb.expected("one_trace", 8)
    j = kb.asked_ops(w).index(-1)
    assert e.abn[j, 0] == 1 and not e.abn[j, 1:].any() and e.tot[j].tolist() == [1, int((w.state == 1).sum())]


def test_fault_case_has_many_ties():
    s = kb.summary(kb.window("fault"))
    assert s.live == 1781
    assert s.pairs.count((2, 0)) > 3 and s.pairs.count((1, 0)) > 100


def test_asked_slots_cover_every_rule():
    for name in kb.WINDOWS + ("fault",):
        w = kb.window(name)
        ops = kb.asked_ops(w)
        e = kb.expected(name, 8)
        assert len(ops) <= kb.K_TOP and -1 in ops and ops.count(ops[0]) == 2
        d = len(ops) - 1 - ops[::-1].index(ops[0])    # the duplicate answers as its first appearance
        for f in kb.FIELDS:
            assert getattr(e, f)[d].tolist() == getattr(e, f)[0].tolist()
        if kb.absent_op(w.table, w.state) is not None:
            assert e.n[len(ops) - 1] == 0 and e.kinds[len(ops) - 1] == 0 and not e.tot[len(ops) - 1].any()
        assert not e.n[len(ops):].any() and (e.trace[len(ops):] == -1).all()
    assert any(kb.absent_op(kb.window(n).table, kb.window(n).state) is not None for n in kb.WINDOWS)


def test_boundary_kinds_have_the_sizes_and_both_sides():
    b = kb.boundary()
    live = kb.live_kinds(b.table, b.state, b.kinds)
    assert sorted(e[0] + e[1] for e in live) == sorted(kb.BOUNDARY_SIZES)
    assert all(e[0] > 0 and e[1] > 0 for e in live if e[0] + e[1] > 1)
    assert b.table.n_traces == sum(kb.BOUNDARY_SIZES) + 40 and int((b.state == 0).sum()) == 40
    # trace-level times: constant within every trace
    for col in (b.table.tstart, b.table.tend):
        lo = np.full(b.table.n_traces, np.iinfo(np.int64).max)
        hi = np.full(b.table.n_traces, np.iinfo(np.int64).min)
        np.minimum.at(lo, b.table.trace, col)
        np.maximum.at(hi, b.table.trace, col)
        assert (lo == hi).all()


def test_oracle_order_is_total():
    for name in ("ties", "fault"):
        w = kb.window(name)
        live = kb.live_kinds(w.table, w.state, w.kinds)
        assert len({e[2] for e in live}) == len(live)   # rep is unique per kind
