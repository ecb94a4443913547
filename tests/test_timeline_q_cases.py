"""CPU checks of the timeline-quantile oracle (tests/timeline_q_cases.py) against the two oracles it must agree
with, and of the classes the GPU test walks through: it must not be able to pass on empty classes."""
import numpy as np
import pytest

import latency_cases as lc
import timeline_cases as tc
import timeline_q_cases as tq


@pytest.mark.parametrize("name", tq.NAMES)
def test_implied_counts_equal_the_timeline_oracle(name):
    for B, what, method in tq.CASES:
        _, cnt = tq.expected(name, B, what, method)
        assert cnt.tolist() == tc.expected(name, B, what).cnt.tolist(), (B, what, method)
    for kind in ("off",):   # a grid that leaves rows before and after: they get no class
        _, cnt = tq.expected(name, 7, "self", "linear", kind)
        e = tc.expected(name, 7, "self", kind)
        assert cnt.tolist() == e.cnt.tolist() and e.out.any()


@pytest.mark.parametrize("grid", ["main", "ns"])
def test_boundary_counts_equal_the_timeline_oracle(grid):
    for what in tc.WHATS:
        _, cnt = tq.boundary_expected(grid, what, "linear")
        assert cnt.tolist() == tc.boundary_expected(grid, what).cnt[tq.boundary_kept(what)].tolist()
    assert tq.boundary_asked("duration") == [c for c in tc.boundary_ops() if c != tc.WRAP]   # the issue's list


@pytest.mark.parametrize("method", tq.METHODS)
@pytest.mark.parametrize("what", tc.WHATS)
def test_one_bucket_equals_the_latency_oracle(what, method):
    """B = 1 on the default grid holds every start of the window: a pod-op's two classes are mr_windows_latency's."""
    for name in tq.NAMES:
        w = tc.window(name)
        asked = tc.asked_ops(w)
        q, cnt = tq.expected(name, 1, what, method)
        ops = [c for c in asked if c >= 0]
        out, count = lc.latency_oracle(w.table, w.state, w.t0, w.t1, ops, what, tq.QS, method)
        rows = [j for j, c in enumerate(asked) if c >= 0]
        assert cnt[rows, 0].tolist() == count.tolist(), name
        assert lc.hexes(q[rows, 0]) == lc.hexes(out), name
        assert count.sum() > 0


def test_class_sizes_of_the_named_cases():
    """Every named window meets, among the classes the GPU test compares on it, a class of 0, of 1 and of 2 values
    and one of 100 or more.  `ragged` (130 traces, 1,181 rows) cannot: its largest class, the window's own traces
    on one side in one bucket, holds 65 values; it must show that one.  Classes of 100 and more, up to 3,000, come
    from the other four windows and from the boundary table."""
    for name in tq.NAMES:
        seen = {0: False, 1: False, 2: False, 100: False}
        largest = 0
        for B, what, method in tq.CASES:
            _, cnt = tq.expected(name, B, what, method)
            for k, v in tq.class_sizes(cnt).items():
                seen[k] = seen[k] or v
            largest = max(largest, int(cnt.max()))
        if name == "ragged":
            assert largest == 65 and seen[0] and seen[1] and seen[2]
        else:
            assert all(seen.values()), (name, seen)
    for grid in ("main", "ns"):
        _, cnt = tq.boundary_expected(grid, "self", "linear")
        sizes = tq.class_sizes(cnt)
        assert sizes[0] and sizes[1] and sizes[2]
    assert int(tq.boundary_expected("main", "self", "linear")[1].max()) == 3000


def test_values_differ_between_methods_and_sides():
    """The oracle is not a constant: the methods disagree somewhere, and so do the two sides."""
    lin, _ = tq.expected("fault", 7, "self", "linear")
    low, _ = tq.expected("fault", 7, "self", "lower")
    high, cnt = tq.expected("fault", 7, "self", "higher")
    assert (low <= lin).all() and (lin <= high).all() and (low < high).any()
    both = (cnt[:, :, 0] > 0) & (cnt[:, :, 1] > 0)
    assert both.any() and (lin[:, :, 0][both] != lin[:, :, 1][both]).any()
    assert not np.isnan(lin).any()
