"""CPU checks of the replica tests' own oracle (tests/replica_cases.py): the figures of its cases, its
invariants against the latency oracle, and brute-force Python loops on the boundary table."""
import numpy as np
import pytest

import kind_breakdown_cases as kb
import latency_cases as lc
import replica_cases as rc
from replica_cases import BIG, K_TOP


def test_pods3_figures():
    w = rc.pods3()
    t = w.table
    assert (t.n_spans, t.n_podops, t.n_svcops) == (36513, 120, 40)
    sv, bad = rc.sv_map(t)
    assert bad.size == 0 and (sv >= 0).all() and np.bincount(sv, minlength=40).tolist() == [3] * 40
    assert (int((w.state == 2).sum()), int((w.state == 1).sum())) == (177, 1823)
    top = rc.top_by_abnormal_rows(t, w.state)
    assert len(top) == K_TOP == 11 and len({int(sv[p]) for p in top}) == 5   # asked entries share slots
    ops = rc.asked("pods3")
    slots = {int(sv[p]) for p in ops}
    assert sum(int((sv == s).sum()) for s in slots) * 2 <= 1024                # keys <= 1024: the direct-mapped table
    sib = ops[len(top) + 1]                 # the first op again, then a replica of an already asked op
    assert ops[len(top)] == ops[0] and sib not in top and sv[sib] in {int(sv[p]) for p in top}


def test_wide_figures():
    w = rc.wide()
    t = w.table
    sv, bad = rc.sv_map(t)
    per = np.bincount(sv[sv >= 0], minlength=t.n_svcops)
    assert t.n_spans == 2215 and int((sv >= 0).sum()) == 743 and bad.size == 0
    assert t.n_svcops == 12 and per.min() == 49 and per.max() == 69           # more than a wave, more than m = 32
    assert (int((w.state == 2).sum()), int((w.state == 1).sum())) == (84, 216)
    ops = rc.wide_ops(w)
    assert len(ops) == 12 and sorted(int(sv[p]) for p in ops) == list(range(12))
    assert per.sum() * 2 >= 1176 > 1024                                         # the hashed table
    c, _, _ = rc.podop_counts(t, w.state, "duration", w.t0, w.t1)
    ties = []
    for s in range(12):                                                          # the code tie key decides
        order = rc.ordered_live(c, rc.replicas_of(sv, s))
        pairs = [(int(c[q, 1]), int(c[q, 0])) for q in order]
        ties.append(len(pairs) - len(set(pairs)))
    # (live replicas whose (abnormal, normal) pair repeats an earlier one's: 35..50 of a list's 49..69)
    assert ties == [45, 45, 35, 50, 45, 44, 47, 47, 40, 45, 45, 44]
    h = rc.wide(half=True)
    assert h.table is t and h.t1 < w.t1 and (h.state > 0).sum() < (w.state > 0).sum()
    e = rc.replica_oracle(t, h.state, ops, 12, 8, "self", h.t0, h.t1)
    assert (e.live < e.all).all() and (e.live > 0).any()


def test_one_pod_figures():
    w = rc.one_pod()
    assert w.pods == [115, 117, 119] and w.state.tolist() == rc.pods3().state.tolist()
    e = rc.replica_oracle(w.table, w.state, [117], 1, 8, "self", w.t0, w.t1)
    assert e.pod[0, :3].tolist() == [115, 119, 117] and e.n[0] == 3
    assert e.cnt[0, :3, ::-1].tolist() == [[228, 438], [0, 415], [0, 433]]      # (abnormal, normal)
    assert (int(e.place[0]), int(e.live[0]), int(e.all[0])) == (2, 3, 3)
    assert e.own[0, :, 0].tolist() == [433, 0] and e.tot[0, :, 0].tolist() == [438 + 415 + 433, 228]


def test_ambiguous_and_span_times():
    a = rc.ambiguous()
    _, bad = rc.sv_map(a.table)
    assert bad.tolist() == [a.pod] and len(set(a.svcs)) == 2
    s = rc.span_times()
    per_trace = [np.unique(s.table.tstart[s.table.trace == t]).size for t in range(8)]
    assert max(per_trace) > 1 and (s.state == 1).any() and (s.state == 2).any()
    sv, bad = rc.sv_map(s.table)
    assert bad.size == 0 and np.bincount(sv[sv >= 0]).max() == 2


@pytest.mark.parametrize("name", ["pods3", "wide", "one_pod"])
def test_invariants(name):
    w = rc.CASES[name]()
    ops = rc.asked(name)
    sv, _ = rc.sv_map(w.table)
    assert len(ops) <= 64 and len(ops) != len(set(ops))
    for what in rc.WHATS:
        e = rc.expected(name, 32, what)
        small = rc.expected(name, 1, what)
        _, count = lc.latency_oracle(w.table, w.state, w.t0, w.t1, ops, what, [0.5], "linear")
        assert e.own[:, :, 0].tolist() == count.tolist()                        # the op's own count: the latency entry's
        for j, p in enumerate(ops):
            listed = e.pod[j, :e.n[j]].tolist()
            assert all(sv[q] == sv[p] for q in listed) and len(set(listed)) == len(listed)
            assert small.pod[j, 0] == e.pod[j, 0] and small.place[j] == e.place[j] and small.tot[j].tolist() == e.tot[j].tolist()
            if 0 <= e.place[j] < e.n[j]:
                assert e.pod[j, e.place[j]] == p and e.cnt[j, e.place[j]].tolist() == e.own[j, :, 0].tolist()
            if e.live[j] <= 32:
                assert e.tot[j, :, 0].tolist() == e.cnt[j].sum(axis=0).tolist()
            for i in range(j):                                                    # one service-op: one list, one total
                if sv[ops[i]] == sv[p] and sv[p] >= 0:
                    assert e.pod[i].tolist() == e.pod[j].tolist() and e.tot[i].tolist() == e.tot[j].tolist()
        gone = kb.absent_op(w.table, w.state)
        if gone is not None:
            j = ops.index(gone)
            assert e.place[j] == -1 and not e.own[j].any()


def test_boundary_table_against_brute_force():
    b = rc.boundary()
    t = b.table
    assert [int(x) for x in np.flatnonzero(b.state == 2)] == list(rc.T_ABN)
    assert [int(x) for x in np.flatnonzero(b.state == 1)] == list(rc.T_NOR)
    assert b.state[rc.T_DROP] == 0 and b.state[rc.T_OUT] == 0
    assert t.n_podops == rc.N_PODS and rc.NEVER not in t.podop and rc.sv_map(t)[0][rc.NEVER] == -1
    ops = rc.boundary_ops()
    at = {c: ops.index(c) for c in set(ops)}
    for what in rc.WHATS:
        for m in (1, 2, 32):
            e = rc.replica_oracle(t, b.state, ops, len(ops), m, what, b.t0, b.t1)
            for j, p in enumerate(ops):
                live, every = rc.brute_force(t, b.state, p, what, b.t0, b.t1)
                assert (int(e.live[j]), int(e.all[j]), int(e.n[j])) == (len(live), every, min(m, len(live)))
                assert e.pod[j, :e.n[j]].tolist() == [x[0] for x in live[:m]]
                for r, x in enumerate(live[:m]):
                    assert (e.cnt[j, r].tolist(), e.sum[j, r].tolist(), e.max[j, r].tolist()) == (x[1], x[2], x[3])
                codes = [x[0] for x in live]
                assert e.place[j] == (codes.index(p) if p in codes else -1)
                for side in (0, 1):
                    on = [x[3][side] for x in live if x[1][side]]
                    assert e.tot[j, side].tolist() == [sum(x[1][side] for x in live), rc.wrap(sum(x[2][side] for x in live)),
                                                       max(on) if on else 0]
    e = rc.replica_oracle(t, b.state, ops, len(ops), 8, "duration", b.t0, b.t1)
    sizes = list(rc.BOUNDARY_SIZES)
    for i, n in enumerate(sizes):                                                # the runs: [normal, abnormal] per replica
        j = at[rc.RUN_A + 2 * i]
        got = {int(q): e.cnt[j, r].tolist() for r, q in enumerate(e.pod[j, :2])}
        assert got == {rc.RUN_A + 2 * i: [sizes[(i + 3) % 10], n], rc.RUN_A + 2 * i + 1: [sizes[(i + 4) % 10], sizes[(i + 1) % 10]]}
    j = at[rc.IL1]
    assert e.pod[j, :2].tolist() == [rc.IL1, rc.IL2] and e.cnt[j, :2].tolist() == [[300, 300], [300, 300]]   # a tie: the code decides
    assert e.place[at[rc.IL2]] == 1 and e.pod[len(ops) - 1].tolist() == e.pod[j].tolist()                     # asked twice
    j = at[rc.WR_UP]                          # sums leave int64 and wrap; WR_DOWN's maximum is negative
    assert e.pod[j, :3].tolist() == [rc.WR_PAR, rc.WR_UP, rc.WR_DOWN] and e.all[j] == 3 and e.place[j] == 1   # (11, 3, 0 abnormal rows)
    assert e.sum[j, 1].tolist() == [0, rc.wrap(3 * BIG + 21)] == [0, -BIG + 21] and e.max[j, 1].tolist() == [0, BIG + 14]
    assert e.sum[j, 2].tolist() == [rc.wrap(-3 * BIG - 15), 0] == [BIG - 15, 0] and e.max[j, 2].tolist() == [-BIG, 0]
    assert e.place[at[rc.WR_DOWN]] == 2 and e.own[at[rc.WR_DOWN], 0].tolist() == [3, BIG - 15, -BIG]
    j = at[rc.DR_DEAD]                        # rows only on the dropped and the outside trace: not live
    assert (int(e.live[j]), int(e.all[j]), int(e.place[j])) == (1, 2, -1) and e.pod[j, :2].tolist() == [rc.DR_LIVE, -1]
    assert not e.own[j].any()
    j = at[rc.NEVER]                          # a code without rows: the padding
    assert (int(e.live[j]), int(e.all[j]), int(e.place[j]), int(e.n[j])) == (0, 0, -1, 0) and (e.pod[j] == -1).all()
    s = rc.replica_oracle(t, b.state, ops, len(ops), 8, "self", b.t0, b.t1)
    assert s.own[at[rc.WR_PAR], 1, 2] == rc.wrap(100 - (3 * BIG + 21)) == BIG + 79   # a wrapped self time, the largest by far
    assert rc.replica_oracle(t, None, ops, len(ops), 8, "self").all.tolist() == [0] * len(ops)
