"""CPU checks of the call-evidence cases (tests/call_edge_cases.py): the shapes that make the GPU cases of
tests/test_gpu_call_edges.py meaningful, and the anchor of the semantics -- the oracle's calls per edge are
the multiplicities of the reference's operation_operation -- on the numpy oracle alone (no GPU needed)."""
import collections
import os

import numpy as np
import pandas as pd
import pytest

import call_edge_cases as ce
import oracle as orc
from conftest import GOLDEN, load_golden, regen_window


def _runs(keys):
    """Lengths of the runs of equal consecutive keys."""
    keys = np.asarray(keys)
    cut = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1], True])
    return np.diff(cut)


def test_named_windows_have_calls_on_both_sides():
    for name in ce.WINDOWS + ("fault",):
        w = ce.window(name)
        ed = ce.edges(name)
        assert sum(int(v[0][1]) for v in ed.values()) > 0 and sum(int(v[0][0]) for v in ed.values()) > 0, name
        ops = ce.asked_ops(w)
        e = ce.expected(name, 8)
        assert 2 <= len(ops) <= ce.K_TOP and ops.count(ops[0]) == 2
        d = len(ops) - 1 - ops[::-1].index(ops[0])    # the duplicate answers as its first appearance
        for f in ce.FIELDS:
            assert getattr(e, f)[d].tolist() == getattr(e, f)[0].tolist()
        assert not e.n[len(ops):].any() and (e.peer[len(ops):] == -1).all()
        assert e.peers.sum() > 0
    # m = 1 truncates somewhere, m = 32 pads somewhere
    assert any((ce.expected(n, 1).peers > 1).any() for n in ce.WINDOWS)
    assert any(((ce.expected(n, 32).n > 0) & (ce.expected(n, 32).n < 32)).any() for n in ce.WINDOWS)


def test_boundary_partition_and_times():
    b = ce.boundary()
    assert np.flatnonzero(b.state == 2).tolist() == list(ce.T_ABN)
    assert np.flatnonzero(b.state == 1).tolist() == list(ce.T_NOR)
    assert b.state[ce.T_OUT] == 0 and b.state[ce.T_DROP] == 0
    inw = (b.table.tstart >= b.t0) & (b.table.tend <= b.t1)
    assert not inw[b.table.trace == ce.T_OUT].any() and inw[b.table.trace == ce.T_DROP].all()
    for col in (b.table.tstart, b.table.tend):   # trace-level times
        for t in range(10):
            assert np.unique(col[b.table.trace == t]).size == 1


def test_boundary_runs_and_interleaving():
    b = ce.boundary()
    child, par, side = ce.call_pairs(b.table, b.state, b.t0, b.t1)
    key = (b.table.podop[par].astype(np.int64) << 32 | b.table.podop[child]) * 2 + side
    by_row = np.full(b.table.n_spans, -1, np.int64)       # a row's (edge, side) as a child, -1: no pair
    by_row[child] = key
    sizes = list(ce.BOUNDARY_SIZES)
    ns = len(sizes)
    for t, sd, shift in ((0, 1, 0), (1, 0, 3)):           # the runs: consecutive rows, every size
        rows = np.flatnonzero(b.table.trace == t)[:-1]    # (without the anchor)
        assert (np.diff(rows) == 1).all()
        r = _runs(by_row[rows])
        got = [int(n) for n, k in zip(r, by_row[rows][np.cumsum(r) - 1]) if k >= 0]
        assert got == [sizes[(i + shift) % ns] for i in range(ns)]
    # runs start at offsets that are no multiple of a wave and cross block tiles (1024 rows)
    first = int(np.flatnonzero(b.table.trace == 0)[0])
    starts = first + np.cumsum([0] + [s + 1 for s in sizes[:-1]]) + 1
    assert (starts % 64 != 0).sum() >= 8 and any(s // 1024 != (s + n - 1) // 1024 for s, n in zip(starts, sizes))
    rows = np.flatnonzero(np.isin(b.table.trace, (2, 3)))[:-2]
    r = _runs(by_row[rows])
    paired = by_row[rows][np.cumsum(r) - 1] >= 0
    assert r[paired].max() == 1 and paired.sum() > 2000    # the same edges, no run of pairs longer than 1
    ed = ce.edge_counts(b.table, b.state, b.t0, b.t1)
    for i in range(ns):
        cap = min(sizes[i], ce.INTERLEAVE_CAP)
        assert ed[(ce.PA + i, ce.CH + i)][0].tolist() == [sizes[(i + 3) % ns] + cap, sizes[i] + cap]


def test_boundary_join_rules():
    b = ce.boundary()
    ed = ce.edge_counts(b.table, b.state, b.t0, b.t1)
    # one spanID on three rows: an abnormal child pairs with the two abnormal rows only
    assert ed[(ce.U1, ce.V)][0].tolist() == [0, 1] and ed[(ce.U2, ce.V)][0].tolist() == [0, 1]
    assert ed[(ce.U3, ce.V)][0].tolist() == [1, 0]
    assert ed[(ce.U1, ce.V)][1].tolist() == [0, 400] and ed[(ce.U1, ce.V)][2].tolist() == [0, 400]
    # the pair exists in the table, and is dead in the window: other side, outside, dropped
    sp = {int(s): int(o) for s, o in zip(b.table.span, b.table.podop)}
    for par, ch in ((ce.W1, ce.W2), (ce.OP, ce.OC), (ce.DP, ce.DC)):
        c = int(np.flatnonzero(b.table.podop == ch)[0])
        assert sp[int(b.table.parent[c])] == par and (par, ch) not in ed
    orphan = int(np.flatnonzero(b.table.podop == ce.ORPH)[0])
    assert b.table.parent[orphan] == -1 and not any(ce.ORPH in k for k in ed)
    assert ed[(ce.SELF, ce.SELF)][0].tolist() == [2, 2] and ed[(ce.SELF, ce.SELF)][2][0] > 0
    assert not any(ce.LONELY in k for k in ed) and (b.table.podop == ce.LONELY).sum() == 10
    assert not (b.table.podop == ce.NEVER).any()


def test_boundary_hub_ties_and_truncation():
    e = ce.boundary_expected()
    asked = ce.boundary_ops()
    j = asked.index(ce.HUB)
    assert asked.count(ce.HUB) == 2
    for f in ce.FIELDS:                                    # the duplicate answers as its first appearance
        assert getattr(e, f)[len(asked) - 1].tolist() == getattr(e, f)[j].tolist()
    for d, base in ((0, ce.Q), (1, ce.CC)):
        assert e.peers[j, d] == ce.NPEER > 32 == e.n[j, d]
        want = sorted(range(ce.NPEER), key=lambda x: (-ce.hub_calls(x)[0], ce.hub_calls(x)[1], x))
        assert e.peer[j, d].tolist() == [base + x for x in want[:32]]
        assert e.calls[j, d, :, 1].tolist() == [ce.hub_calls(x)[0] for x in want[:32]]
        assert e.calls[j, d, :, 0].tolist() == [ce.hub_calls(x)[1] for x in want[:32]]
        # the totals cover all 40 peers, not the 32 listed
        assert e.tot[j, d].tolist() == [sum(ce.hub_calls(x)[1] for x in range(ce.NPEER)),
                                        sum(ce.hub_calls(x)[0] for x in range(ce.NPEER))]
        assert e.tot[j, d, 1] > e.calls[j, d, :, 1].sum()
    keys = [ce.hub_calls(x) for x in range(ce.NPEER)]
    assert keys[0] == keys[12] and len(set(keys)) < ce.NPEER      # ties down to the code
    for name in (ce.LONELY, ce.NEVER, ce.ORPH):            # asked ops with no call at all
        jj = asked.index(name)
        assert not e.n[jj].any() and not e.peers[jj].any() and not e.tot[jj].any() and (e.peer[jj] == -1).all()
    assert e.peer[asked.index(ce.SELF), 0, 0] == ce.SELF == e.peer[asked.index(ce.SELF), 1, 0]   # a self edge: both


def test_boundary_durations_wrap_and_go_negative():
    b = ce.boundary()
    ed = ce.edge_counts(b.table, b.state, b.t0, b.t1)
    child, par, side = ce.call_pairs(b.table, b.state, b.t0, b.t1)
    for i, sd in ((ce.WRAP_UP, 1), (ce.WRAP_DOWN, 0)):
        m = (b.table.podop[par] == ce.PA + i) & (b.table.podop[child] == ce.CH + i) & (side == sd)
        true = sum(int(x) for x in b.table.duration[child[m]])
        calls, dsum, dmax = ed[(ce.PA + i, ce.CH + i)]
        assert calls[sd] == m.sum() > 64
        assert not -(1 << 63) <= true < (1 << 63)                       # the true sum leaves int64 ...
        assert int(dsum[sd]) == (true + (1 << 63)) % (1 << 64) - (1 << 63)   # ... and the oracle's wraps
    assert ed[(ce.PA + ce.WRAP_DOWN, ce.CH + ce.WRAP_DOWN)][2][0] < -ce.BIG // 2   # a negative maximum
    assert ed[(ce.PA + ce.WRAP_UP, ce.CH + ce.WRAP_UP)][2][1] > ce.BIG


def test_wide_table_is_past_the_layout_limit():
    w = ce.wide()
    assert w.table.n_podops == 4100 > 4096 and 3000 < w.table.n_spans < 10_000
    assert int((w.state == 2).sum()) == 1025 == int((w.state == 1).sum())
    e = ce.call_oracle(w.table, w.state, ce.WIDE_ASKED, len(ce.WIDE_ASKED), 8, w.t0, w.t1)
    assert e.peers[:, 0].tolist() == [1] * len(ce.WIDE_ASKED) == e.peers[:, 1].tolist()
    assert e.peer[ce.WIDE_ASKED.index(4099), :, 0].tolist() == [4098, 0]


def _oo_counts(table, sel):
    sg = orc.span_graph(table.trace, table.podop, table.span, table.parent, sel)
    oo = orc.span_graph_dicts(sg, table.span, table.parent, table.podop_names, table.trace_names)[0]
    return {a: collections.Counter(lst) for a, lst in oo.items() if lst}


@pytest.mark.parametrize("source", ["edges_spans", "pods_dup_broken"])
def test_anchor_calls_are_operation_operation_multiplicities(source):
    """For each side's trace list, calls[edge][side] == the multiplicity of the child in
    operation_operation[parent] that the reference builds from that list (oracle.span_graph_dicts)."""
    from microrank_amd.spans import SpanTable

    if source == "edges_spans":
        table = SpanTable.from_dataframe(pd.read_parquet(os.path.join(GOLDEN, "edges_spans.parquet")))
        rng = np.random.default_rng(5)
        state = rng.integers(0, 3, table.n_traces).astype(np.uint8)      # any partition: 0 out, 1 normal, 2 abnormal
    else:
        c = load_golden("pods_dup_broken.json")
        _, adf = regen_window(c)
        table = SpanTable.from_dataframe(adf)
        state = ce.kb.state_of(table.n_traces, c["detect"]["abnormal"], c["detect"]["normal"])
    assert (state == 1).any() and (state == 2).any()
    ed = ce.edge_counts(table, state)
    names = table.podop_names
    total = 0
    for side in (0, 1):
        got = {}
        for (a, b), v in ed.items():
            if v[0][side]:
                got.setdefault(names[a], collections.Counter())[names[b]] = int(v[0][side])
        want = _oo_counts(table, state == side + 1)
        assert got == want
        total += sum(sum(c.values()) for c in want.values())
    assert total > (100 if source == "pods_dup_broken" else 10)   # (edges_spans is a table of a few dozen spans)
    # duplicated spanIDs fan out and broken parents make no pair (T11), in the golden table itself
    child, par, _ = ce.call_pairs(table, np.full(table.n_traces, 2, np.uint8))
    if source == "pods_dup_broken":
        assert np.bincount(child).max() > 1
        assert (table.parent >= 0).sum() > np.unique(child).size or (table.parent < 0).sum() > table.n_traces
