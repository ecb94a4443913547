"""CPU checks of the timeline tests' own oracle (tests/timeline_cases.py): its invariants against the latency
oracle and the detector's counts on the five windows, and hand-written numbers on the boundary table."""
import numpy as np
import pytest

import latency_cases as lc
import timeline_cases as tc
from timeline_cases import B0, BIG, BW, I64_MIN, K_TOP, NB


@pytest.mark.parametrize("name", tc.NAMES)
def test_invariants_on_the_five_windows(name):
    w = tc.window(name)
    asked = tc.asked_ops(w)
    assert -1 in asked and len(asked) != len(set(asked)) and len(asked) <= K_TOP
    for what in tc.WHATS:
        _, count = lc.latency_oracle(w.table, w.state, w.t0, w.t1, [max(c, 0) for c in asked], what, [0.5], "linear")
        for B, kind in ((1, "default"), (7, "off"), (30, "default"), (30, "off"), (512, "off")):
            e = tc.expected(name, B, what, kind)
            total = e.cnt.sum(axis=1) + e.out.sum(axis=2)           # [K, side]
            for j, c in enumerate(asked):
                if c < 0:   # the window's own timeline: the state's counts
                    assert total[j].tolist() == [int((w.state == 1).sum()), int((w.state == 2).sum())]
                else:
                    assert total[j].tolist() == count[j].tolist(), (what, B, kind, c)
            assert not total[len(asked):].any() and not e.max[e.cnt == 0].any() and not e.sum[e.cnt == 0].any()
            if kind == "default":   # every start of [t0, t1] is in a bucket
                assert not e.out.any()
            elif B > 1:
                assert e.out[:, :, 0].any() and e.out[:, :, 1].any() and e.cnt.any()
    first = asked.index(asked[0], 1)                                  # the repeated op: answered each time
    e = tc.expected(name, 30, "self")
    assert e.cnt[first].tolist() == e.cnt[0].tolist() and e.cnt[0].sum() > 0
    if len(asked) > first + 1:                                        # the absent op: zeros
        assert not e.cnt[first + 1].any() and not e.out[first + 1].any()


def test_bucket_arithmetic():
    assert tc.bucket_of(B0, B0, BW, NB) == 0 and tc.bucket_of(B0 - 1, B0, BW, NB) == NB
    assert tc.bucket_of(B0 + NB * BW - 1, B0, BW, NB) == NB - 1 and tc.bucket_of(B0 + NB * BW, B0, BW, NB) == NB + 1
    assert tc.bucket_of(5, I64_MIN, BIG, 4) == 2 and tc.bucket_of(5, I64_MIN, BIG, 2) == 3
    assert tc.bucket_of(-1, I64_MIN, BIG, 4) == 1 and tc.bucket_of(I64_MIN, I64_MIN, 1, 1) == 0
    assert tc.bucket_of(tc.I64_MAX, I64_MIN, 1, 512) == 513 and tc.bucket_of(tc.I64_MAX, I64_MIN, tc.I64_MAX, 3) == 2


def test_boundary_table_by_hand():
    b = tc.boundary()
    assert [int(t) for t in np.flatnonzero(b.state == 2)] == list(tc.T_ABN)
    assert [int(t) for t in np.flatnonzero(b.state == 1)] == list(tc.T_NOR)
    assert b.state[tc.T_DROP] == 0 and b.state[tc.T_OUT] == 0
    asked = tc.boundary_ops()
    at = {c: asked.index(c) for c in set(asked)}
    e = tc.boundary_expected("main", "duration")
    # EDGE: two rows of (t + 1) * 10 + {0, 1} in trace t; traces 0 / 1 start on b0, 2 / 3 one ns before it,
    # 4 / 5 on the last ns of the last bucket, 6 / 7 one ns after it; the dropped and the outside trace add nothing
    j = at[tc.EDGE]
    assert e.cnt[j].tolist() == [[2, 2], [0, 0], [0, 0], [2, 2]]
    assert e.sum[j].tolist() == [[41, 21], [0, 0], [0, 0], [121, 101]]
    assert e.max[j].tolist() == [[21, 11], [0, 0], [0, 0], [61, 51]]
    assert e.out[j].tolist() == [[2, 2], [2, 2]]
    assert all(getattr(e, f)[len(asked) - 2].tolist() == getattr(e, f)[j].tolist() for f in tc.FIELDS)   # asked twice
    # -1: one trace per side on every edge, two per side in bucket 1 (runs 8 / 9, wraps 14 / 15), a trace is
    # worth 500 + its code
    j = at[-1]
    assert e.cnt[j].tolist() == [[1, 1], [2, 2], [1, 1], [1, 1]] and e.out[j].tolist() == [[1, 1], [1, 1]]
    assert e.sum[j].tolist() == [[501, 500], [509 + 515, 508 + 514], [511, 510], [505, 504]]
    assert e.max[j].tolist() == [[501, 500], [515, 514], [511, 510], [505, 504]]
    # WRAP: three rows of 2^62 + 7k (abnormal, trace 14 on the first ns of bucket 1) and of -2^62 - 5k (normal,
    # trace 15 on its last ns): the sums leave int64 and wrap, the normal maximum is negative
    j = at[tc.WRAP]
    assert e.cnt[j].tolist() == [[0, 0], [3, 3], [0, 0], [0, 0]] and not e.out[j].any()
    assert e.sum[j][1].tolist() == [BIG - 15, -BIG + 21] == [tc.wrap(-3 * BIG - 15), tc.wrap(3 * BIG + 21)]
    assert e.max[j][1].tolist() == [-BIG, BIG + 14]
    j = at[tc.NEG]                       # -5, -9, -2: every value of the bucket is negative
    assert e.cnt[j][1].tolist() == [3, 0] and e.sum[j][1].tolist() == [-16, 0] and e.max[j][1].tolist() == [-2, 0]
    # the runs: one key each, BOUNDARY_SIZES rows (the normal trace's shifted by three), all in bucket 1
    sizes = list(tc.BOUNDARY_SIZES)
    for i, n in enumerate(sizes):
        j = at[tc.RUN + i]
        assert e.cnt[j].tolist() == [[0, 0], [sizes[(i + 3) % len(sizes)], n], [0, 0], [0, 0]]
    for op in (tc.IL1, tc.IL2):          # interleaved: bucket 2, both sides
        assert e.cnt[at[op]].tolist() == [[0, 0], [0, 0], [tc.INTERLEAVED, tc.INTERLEAVED], [0, 0]]
    assert not e.cnt[at[tc.NEVER]].any() and e.cnt[at[tc.LON]].sum() + e.out[at[tc.LON]].sum() == 14
    # self time: a run's parent loses its children's durations, a child keeps its own; the WRAP parents lose
    # a wrapped sum
    s = tc.boundary_expected("main", "self")
    d = b.table.duration
    assert s.sum[at[tc.RUN]].tolist() == e.sum[at[tc.RUN]].tolist()
    def runs_parents(t):   # the summed self time of trace t's PAR rows: their durations less their children's
        return (sum(int(x) for x in d[(b.table.trace == t) & (b.table.podop == tc.PAR)]) -
                sum(int(x) for x in d[(b.table.trace == t) & (b.table.podop >= tc.RUN)]))

    par14, par15 = 100 - (3 * BIG + 21), 100 - (-3 * BIG - 15)
    assert s.cnt[at[tc.PAR]][1].tolist() == [11, 11]
    assert s.sum[at[tc.PAR]][1].tolist() == [tc.wrap(runs_parents(9) + par15), tc.wrap(runs_parents(8) + par14)]
    assert s.max[at[tc.PAR]][1, 1] == tc.wrap(par14) == BIG + 79   # (the wrapped self time is the largest by far)
    # the other grids: one-ns buckets; the widest buckets from the smallest origin
    n = tc.boundary_expected("ns", "duration")
    j = at[tc.EDGE]
    assert n.cnt[j][0].tolist() == [2, 2] and n.cnt[j].sum() == 4 and n.out[j].tolist() == [[2, 4], [2, 4]]
    w4, w2 = tc.boundary_expected("wide4", "duration"), tc.boundary_expected("wide2", "duration")
    assert w4.cnt[j].tolist() == [[0, 0], [0, 0], [8, 8], [0, 0]] and not w4.out.any()
    assert not w2.cnt.any() and w2.out[j].tolist() == [[0, 8], [0, 8]]
