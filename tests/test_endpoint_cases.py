"""CPU checks of the endpoint tests' own cases (tests/endpoint_cases.py): each case has the property it is named
for, and the vectorised oracle agrees with plain loops (no GPU, no library)."""
import numpy as np
import pytest

import detect_cases as dc
import endpoint_cases as ec


def test_index_rules_by_hand():
    w = ec.index()
    t = w.table
    assert ec.entry_ops(t).tolist() == ec.IX_EXPECT == ec.entry_ops_loops(t)
    rows = ec.entry_rows(t)
    later = np.flatnonzero(t.trace == ec.IX_LATER)
    assert rows[ec.IX_LATER] == later[1] and t.duration[later[1]] > t.duration[later[0]]
    tie = np.flatnonzero(t.trace == ec.IX_TIE)
    assert t.duration[tie[0]] == t.duration[tie[1]] and rows[ec.IX_TIE] == tie[0]
    assert t.duration[rows[ec.IX_NEG]] < 0 and t.duration[t.trace == ec.IX_NEG].max() > 0
    big = t.duration[t.trace == ec.IX_BIG].tolist()
    assert sorted(big) == [-ec.BIG, ec.BIG - 1, ec.BIG] and t.duration[rows[ec.IX_BIG]] == ec.BIG
    for none in (ec.IX_CYCLE, ec.IX_ELSEWHERE):
        r = np.flatnonzero(t.trace == none)
        assert r.size == 2 and (t.parent[r] >= 0).all() and rows[none] == -1
    a, b = np.flatnonzero(t.trace == ec.IX_CYCLE)
    assert t.parent[a] == t.span[b] and t.parent[b] == t.span[a]                      # the cycle
    assert not np.isin(t.parent[t.trace == ec.IX_ELSEWHERE], t.span[t.trace == ec.IX_ELSEWHERE]).any()
    assert ec.one_row().table.n_spans == 1 and ec.entry_ops(ec.one_row().table).tolist() == [0]


def test_unknown_parent_id_is_a_root():
    from microrank_amd.spans import SpanTable

    t = SpanTable.from_dataframe(ec.unknown_parent_frame())
    assert t.parent.tolist() == [-1, -1, 1]
    assert [t.podop_names[c] for c in ec.entry_ops(t)] == ["p_x", "p_y"]


@pytest.mark.parametrize("name", dc.ORDERS)
def test_interleaved_orders(name):
    w = ec.order_table(name)
    t = w.table
    assert ec.root_spread(t) > 256                                   # a trace's root rows lie more than a block apart
    assert ec.entry_ops(t).tolist() == ec.entry_ops_loops(t)
    roots = np.bincount(t.trace[ec.root_rows(t)], minlength=t.n_traces)
    assert roots.min() >= 1 and roots.max() > 20
    # the same logical rows in every order: the entry row's DURATION is the same, its pod-op may differ only on a tie
    base = ec.order_table("grouped").table
    assert t.duration[ec.entry_rows(t)].tolist() == base.duration[ec.entry_rows(base)].tolist()
    assert set(w.state.tolist()) == {0, 1, 2}


def test_distinct_counts_traces_not_rows():
    w = ec.distinct()
    t = w.table
    spans = [int(((t.trace == tr) & (t.podop == ec.X_D)).sum()) for tr in range(4)]
    assert spans == [1, 2, 70, 0] and w.state.tolist() == [2, 1, 2, 1]
    e = ec.endpoint_oracle(t, w.state, [ec.X_D, ec.E_D, -1], 3, 4)
    assert e.op[:, 0].tolist() == [ec.E_D] * 3 and e.live.tolist() == [1, 1, 1]
    assert e.cnt[0, 0].tolist() == [1, 2] and sum(spans) == 73       # (normal, abnormal) traces, not rows
    assert e.cnt[1, 0].tolist() == e.cnt[2, 0].tolist() == [2, 2]    # the asked op that is the endpoint: every trace


def test_ranked_order_by_hand():
    w = ec.ranked()
    t = w.table
    assert w.state.tolist() == [2, 2, 1, 2, 2, 1, 1, 1, 1, 2, 2, 2, 2, 2, 1, 0]
    e = ec.endpoint_oracle(t, w.state, [-1, ec.X_R, ec.GONE_R], 3, 8)
    # 4: (3, 0); then the tie at (2, 1): codes 1, 2, the traces without a root row last; 3 is normal only
    assert e.op[0, :5].tolist() == [4, 1, 2, ec.NONE, 3] == e.op[1, :5].tolist() and e.live.tolist() == [5, 5, 0]
    assert e.cnt[0, :5, ::-1].tolist() == [[3, 0], [2, 1], [2, 1], [2, 1], [0, 3]]
    assert e.op[2].tolist() == [-1] * 8 and not e.tot[2].any()        # an op with no trace in the window
    for m in (4, 5, 6):                                               # m below, at and above live
        x = ec.endpoint_oracle(t, w.state, [-1], 1, m)
        assert x.n.tolist() == [min(m, 5)] and x.live.tolist() == [5] and x.tot.tolist() == e.tot[:1].tolist()
    states = [ec.state_of(t, a, b) for a, b in ec.ranked_windows()]
    assert states[2] is None and 0 < (states[1] > 0).sum() < (states[0] > 0).sum() and (states[3] > 0).sum() == 12


def test_wide_is_past_the_direct_table():
    w = ec.wide()
    ep = ec.entry_ops(w.table)
    assert np.unique(ep).tolist() == list(range(ec.N_WIDE)) and (ec.N_WIDE + 1) * 2 > ec.EV_H
    assert 2000 < w.table.n_spans < 8000 and set(w.state.tolist()) == {1, 2}
    ops = ec.wide_asked()
    assert len(ops) == 64 and ops.count(-1) == 2 and ops.index(-1) == 32 and len(set(ops)) < 64
    entries = np.unique(np.stack([w.table.trace, w.table.podop], 1), axis=0).shape[0]
    assert entries > 2 * ec.TILE                                      # MR_EP_BLOCKS = 3 gives every block a tile
    assert (3 + 1) * 2 <= ec.EV_H                                     # ranked()'s one slot is direct-mapped


@pytest.mark.parametrize("n", [ec.TILE - 1, ec.TILE, ec.TILE + 1])
def test_cut_sizes(n):
    w = ec.cut(n)
    assert w.table.n_traces == n == w.table.n_spans
    assert np.bincount(w.state, minlength=3).tolist() == [len(range(2, n, 3)), len(range(1, n, 3)), len(range(0, n, 3))]


def test_wrapping_values():
    w = ec.wrapping()
    d = ec.trace_values(w.table)
    assert d == [-(1 << 63)] * 3 + [4] and w.state.tolist() == [2, 2, 1, 2]
    e = ec.endpoint_oracle(w.table, w.state, [-1], 1, 2)
    assert e.sum[0, 0].tolist() == [-(1 << 63), 4] and e.max[0, 0].tolist() == [-(1 << 63), 4]   # 2 * -2^63 + 4 wraps
    assert e.cnt[0, 0].tolist() == [1, 3]


def test_oracle_against_loops():
    """endpoint_oracle's counts against a dict built row by row."""
    w = ec.order_table("random")
    t = w.table
    ep, d = ec.entry_ops_loops(t), ec.trace_values(t)
    for p in (-1, 0, 7):
        acc = {}
        seen = set()
        for r in range(t.n_spans):
            tr = int(t.trace[r])
            if (p >= 0 and int(t.podop[r]) != p) or tr in seen or w.state[tr] == 0:
                continue
            seen.add(tr)
            a = acc.setdefault(ep[tr], [0, 0])
            a[int(w.state[tr]) - 1] += 1
        got = ec.slot_counts(t, w.state, p)
        assert {e: a[0] for e, a in got.items()} == acc and acc
        e = ec.endpoint_oracle(t, w.state, [p], 1, 32)
        assert int(e.tot[0, :, 0].sum()) == len(seen) and int(e.live[0]) == len(acc)
        assert int(e.tot[0, :, 1].sum()) == sum(d[tr] for tr in seen)
