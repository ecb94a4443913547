"""CPU checks of the detector edge cases (detect_cases.py): every case has the property it is named for, so
a builder that loses its teeth fails here instead of passing silently on the GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import detect_cases as dc


def _ulp_apart(a, b):
    return a == b or math.nextafter(a, b) == b


# ---------------------------------------------------------------------------------- A: row order
def test_order_base_shape():
    b = dc.order_base()
    assert b.sizes.size == 40 and sorted(b.sizes.tolist(), reverse=True)[:4] == [300, 65, 64, 63]
    assert {1, 2} <= set(b.sizes.tolist()) and 1300 <= b.trace.size <= 1700
    assert np.unique(b.svcop).size == 9 and np.unique(b.podop).size == 18
    has = b.parent >= 0
    assert has.sum() > 1000
    assert (b.trace[b.parent[has]] == b.trace[has]).all()          # parents inside the trace
    assert (b.tts < 0).any() and (b.rts < 0).any()


@pytest.mark.parametrize("order", dc.ORDERS)
def test_order_is_a_permutation_with_interleaved_traces(order):
    p = dc.order_perm(order)
    b = dc.order_base()
    assert sorted(p.tolist()) == list(range(b.trace.size))
    wave, block, sandwiched = dc.interleaving(b.trace[p])
    if order == "grouped":
        assert (np.diff(b.trace[p]) >= 0).all() and not sandwiched
    else:
        assert wave and block and sandwiched
    if order == "alternating":
        assert len(set(b.trace[p][0:130:2])) == 1 and len(set(b.trace[p][1:130:2])) == 1
        assert b.trace[p][0] != b.trace[p][1]


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("order", dc.ORDERS)
def test_order_tables_have_a_verdict_mix(order, uniform):
    """Both windows hold abnormal, normal and dropped traces; the cut window holds part of the table, and
    with per-span times part of some traces; every order describes the same logical table."""
    t = dc.order_table(order, uniform)
    b = dc.order_base()
    assert dc.uniform_times(t) == uniform
    g = dc.order_table("grouped", uniform)
    whole, cut = dc.order_windows(t)
    for win in (whole, cut):
        state, na, nn, rows = dc.detect_oracle(t, *win, b.a3, b.ok)
        ref = dc.detect_oracle(g, *win, b.a3, b.ok)
        assert state.tolist() == ref[0].tolist() and (na, nn, rows) == ref[1:]
        assert na >= 3 and nn >= 3
        inside = (t.tstart >= win[0]) & (t.tend <= win[1])
        assert (state[np.unique(t.trace[inside])] == 0).any()       # a dropped trace with rows inside
    assert dc.detect_oracle(t, *whole, b.a3, b.ok)[3] == t.n_spans
    state, _, _, rows = dc.detect_oracle(t, *cut, b.a3, b.ok)
    assert 200 < rows < t.n_spans - 200
    if not uniform:
        inside = (t.tstart >= cut[0]) & (t.tend <= cut[1])
        part = [k for k in range(t.n_traces) if 0 < inside[t.trace == k].sum() < (t.trace == k).sum()]
        assert len(part) >= 5
        assert state.tolist() != dc.detect_oracle(t, *whole, b.a3, b.ok)[0].tolist()


def test_append_case_cuts_traces_and_retires_some():
    c1, c2, keep_from, slo = dc.append_case()
    both = set(c1["traceID"]) & set(c2["traceID"])
    start = dict(zip(c1["traceID"], c1["startTime"].astype("int64")))
    kept_cut = [t for t in both if start[t] >= keep_from]
    assert len(kept_cut) >= 3                                        # survive, rows on both sides of the boundary
    retired = [t for t in set(c1["traceID"]) if start[t] < keep_from]
    assert len(retired) >= 3 and any(t not in both for t in retired)
    rows = np.concatenate([c1["traceID"][c1["startTime"].astype("int64") >= keep_from].to_numpy(), c2["traceID"].to_numpy()])
    codes = np.unique(rows, return_inverse=True)[1]
    assert all(dc.interleaving(codes))
    assert len(slo) == dc.ORDER_OPS


# ---------------------------------------------------------------------------------- B: verdict arithmetic
def _case(v, name):
    return v.names.index(name)


def _verdict(v, t, mode="seq"):
    """0 dropped / 1 normal / 2 abnormal of trace t from exact arithmetic."""
    mx = int(v.table.duration[v.table.trace == t].max())
    if mx <= 0:
        return 0
    terms = [(c, a) for c, a, ok in v.terms[t] if ok]
    return 2 if dc.real_of(mx) > dc.expect_exact(terms, mode) else 1


def test_verdict_table_matches_exact_arithmetic():
    """oracle.detect over the whole table gives, for every trace, the verdict of the Fraction model of the
    sequential arithmetic; every kind holds both verdicts."""
    v = dc.verdict_case()
    state, na, nn, rows = dc.detect_oracle(v.table, dc.I64_MIN, dc.I64_MAX, v.a3, v.ok)
    assert rows == v.table.n_spans and 250 <= v.table.n_traces <= 350
    assert state.tolist() == [_verdict(v, t) for t in range(v.table.n_traces)]
    for k in dc.VERDICT_KINDS:
        assert {1, 2} <= set(state[v.kinds == k].tolist()), k
    assert dc.uniform_times(v.table) and not dc.uniform_times(dc.per_span(v.table))
    sizes = np.bincount(v.table.trace)
    assert sizes.max() == 3000


def test_verdict_ties():
    v = dc.verdict_case()
    state = dc.detect_oracle(v.table, dc.I64_MIN, dc.I64_MAX, v.a3, v.ok)[0]
    n = 0
    while f"tie{n}" in v.names:
        t = _case(v, f"tie{n}")
        mx = int(v.table.duration[v.table.trace == t].max())
        real = mx / 1000.0
        assert dc.real_of(mx) == real
        (c, a, _), = v.terms[t]
        assert c == 1 and a == real and state[t] == 1                       # real == expect: normal
        (_, lo, _), = v.terms[_case(v, f"below{n}")]
        (_, hi, _), = v.terms[_case(v, f"above{n}")]
        assert lo == math.nextafter(real, -math.inf) and hi == math.nextafter(real, math.inf)
        assert state[_case(v, f"below{n}")] == 2 and state[_case(v, f"above{n}")] == 1
        n += 1
    assert n >= 5


@pytest.mark.parametrize("kind,other", [("fma", "fused"), ("order", "reverse")])
def test_searched_cases_flip(kind, other):
    """At least 20 stored cases of each kind; recomputed with fractions.Fraction, the sequential sum and
    the other arithmetic fall on opposite sides of real, within an ulp of each other's neighbour; both
    verdicts occur; the table holds them as stored."""
    found = dc.searched_cases()
    assert len(found[kind]) >= 20 and found["draws"] < 400_000
    v = dc.verdict_case()
    verdicts = set()
    for i, (mx, terms) in enumerate(found[kind]):
        assert len(terms) == 2 if kind == "fma" else len(terms) >= 3
        assert 1000 <= mx <= 5_000_000 and all(1 <= c <= 9 and a > 0 for c, a in terms)
        assert all(Fraction(round(a * 10000), 10000) == Fraction(str(round(a, 4))) for _, a in terms)
        assert sum(Fraction(c) * Fraction(round(a * 10000), 10000) for c, a in terms) == Fraction(mx, 1000)
        real, seq, alt = dc.real_of(mx), dc.expect_exact(terms), dc.expect_exact(terms, other)
        assert (real > seq) != (real > alt)
        assert seq != alt and abs(seq - alt) <= 4 * math.ulp(real)
        verdicts.add(real > seq)
        t = _case(v, f"{kind}{i}")
        assert [(c, a) for c, a, _ in v.terms[t]] == terms
        assert _verdict(v, t) != _verdict(v, t, other)
        ops = np.unique(v.table.svcop[v.table.trace == t])
        assert v.a3[ops].tolist() == [a for _, a in terms]                  # name order = the terms' order
        assert np.bincount(v.table.svcop[v.table.trace == t])[ops].tolist() == [c for c, _ in terms]
    assert verdicts == {True, False}


def test_verdict_signs_and_validity():
    v = dc.verdict_case()
    state = dc.detect_oracle(v.table, dc.I64_MIN, dc.I64_MAX, v.a3, v.ok)[0]
    st = lambda name: int(state[_case(v, name)])
    mx = lambda name: int(v.table.duration[v.table.trace == _case(v, name)].max())
    assert (mx("max0"), st("max0")) == (0, 0) and (mx("max_neg"), st("max_neg")) == (-5, 0)
    assert mx("pos_beside_neg") == 9 and st("pos_beside_neg") == 2 and st("pos_beside_neg_n") == 1
    assert (v.table.duration[v.table.trace == _case(v, "pos_beside_neg")] < 0).sum() == 3
    assert mx("max1_tie") == 1 and 1 / 1000.0 == 0.001 and st("max1_tie") == 1 and st("max1_below") == 2
    # ops without an SLO add nothing: adding them would turn each of these verdicts
    assert st("nan_skipped") == 2 and st("huge_skipped") == 2 and st("neg_huge_skipped") == 1
    for name in ("nan_skipped", "huge_skipped", "neg_huge_skipped"):
        t = _case(v, name)
        every = 0.0
        for c, a, _ in v.terms[t]:
            every = every + float(c) * a
        assert (2 if mx(name) / 1000.0 > every else 1) != st(name)
    assert st("none_valid_pos") == 2 and st("none_valid_zero") == 0
    assert st("neg_a3_tie") == 1 and st("neg_a3_over") == 2 and st("neg_expect") == 2
    assert (v.a3[v.ok == 1] < 0).any() and np.isnan(v.a3[v.ok == 0]).any() and (v.a3[v.ok == 0] == 1e300).any()
    for i in range(3):
        (c, a, _), = v.terms[_case(v, f"big{i}")]
        assert c >= 1500 and _ulp_apart(float(c) * a, mx(f"big{i}") / 1000.0)
        assert st(f"big{i}_over") == 2
    assert st("big0") == 1


# ---------------------------------------------------------------------------------- C: window edges
def test_edge_tables():
    table, a3, ok, inside = dc.edge_uniform()
    t0, t1 = dc.EDGE_WIN
    state, na, nn, rows = dc.detect_oracle(table, t0, t1, a3, ok)
    assert ((state > 0) == inside).all() and rows == 2 * inside.sum() and na >= 2 and nn >= 2
    ts, te = table.tstart, table.tend
    for want in ((t0, t1), (t0 - 1, None), (None, t1 + 1), (t0, t0), (t1, t1)):
        assert any((want[0] is None or a == want[0]) and (want[1] is None or b == want[1]) for a, b in zip(ts, te))
    assert dc.detect_oracle(table, t0, t0, a3, ok)[3] == 2 and dc.detect_oracle(table, 100, 200, a3, ok)[0] is None
    table, a3, ok, exp, rows = dc.edge_per_span()
    state, na, nn, got_rows = dc.detect_oracle(table, t0, t1, a3, ok)
    assert state.tolist() == exp.tolist() and got_rows == rows and not dc.uniform_times(table)
    whole = dc.detect_oracle(table, dc.I64_MIN, dc.I64_MAX, a3, ok)[0]
    assert whole.tolist() == [2, 2, 2, 1, 1]                          # the rows outside decide otherwise
    r = table.trace == 0                                              # the inside max against the whole trace's counts
    assert 2500 / 1000.0 <= sum(a3[o] for o in table.svcop[r])
    table, a3, ok = dc.edge_single()
    assert (table.n_traces, table.n_svcops) == (1, 1)
    one = dc.detect_oracle(table, 4, 9, a3, ok)
    assert one[0].tolist() == [2] and one[1:] == (1, 0, 3)


# ---------------------------------------------------------------------------------- D: staging
@pytest.mark.parametrize("name", list(dc.STAGE_TABLES))
def test_stage_tables(name):
    """The first block's entry count, the straddling and the over-long trace, the one-entry blocks; every
    trace's sequential expect is real (odd traces) or one ulp below (even); summing a trace's terms from
    last to first changes the verdict of many traces."""
    nt, first, big = dc.STAGE_TABLES[name]
    s = dc.stage_case(name)
    t = s.table
    assert t.n_traces == nt and t.n_spans < 30_000
    key = np.unique(t.trace.astype(np.int64) * t.n_svcops + t.svcop)
    ent = np.bincount(key // t.n_svcops, minlength=nt)
    assert ent.tolist() == s.entries.tolist() and int(ent[:dc.DB].sum()) == first
    off = np.concatenate([[0], np.cumsum(ent)])
    if first > dc.STAGE:
        assert ((off[:-1][:dc.DB] < dc.STAGE) & (off[1:][:dc.DB] > dc.STAGE)).any()   # a trace straddles the stage edge
    assert (ent.max() >= 4100) == big
    if name == "nt513":
        assert (ent[256:512] == 1).all()
    if nt > dc.DB:
        assert ent[dc.DB] == 1 or name == "nt513"
    assert (t.n_svcops <= 4096) == (not big)
    state = dc.detect_oracle(t, dc.I64_MIN, dc.I64_MAX, s.a3, s.ok)[0]
    assert state.tolist() == s.state.tolist() and set(state.tolist()) <= {1, 2}
    flips = moved = 0
    for k in range(nt):
        ops, cn = np.unique(t.svcop[t.trace == k], return_counts=True)
        terms = [(int(c), float(s.a3[o])) for o, c in zip(ops, cn) if s.ok[o]]
        real = int(t.duration[t.trace == k].max()) / 1000.0
        seq = 0.0
        for c, a in terms:
            seq = seq + float(c) * a
        assert seq == (real if k % 2 else math.nextafter(real, -math.inf))
        rev = 0.0
        for c, a in reversed(terms):
            rev = rev + float(c) * a
        flips += (real > rev) != (real > seq)
        moved += rev != seq
    multi = int((ent > 8).sum())
    assert moved >= max(1, multi // 2) and (flips >= multi // 8 or multi < 16)
    a = np.abs(s.a3[:t.n_svcops - nt])
    assert a.min() < 1e-2 and a.max() > 1e5 and (s.ok[:t.n_svcops - nt] == 0).any()
    assert not dc.uniform_times(dc.per_span(t)) or t.n_spans == 1


# ---------------------------------------------------------------------------------- E: sweep
def test_sweep_cases():
    table, a3, ok = dc.sweep_table()
    assert dc.uniform_times(table) and table.n_traces == 200 and all(dc.interleaving(table.trace))
    ts, te = table.tstart, table.tend
    assert ts.min() < 0 and ts.max() > 4096 * 7 and (te - ts > 20).any() and ((te == ts) & (ts % 7 == 0)).sum() >= 30
    assert {(7, 20), (7, 0)} <= {(g, w) for _, g, w, _ in dc.SWEEPS}
    assert {0, 1, 4096, 4097} <= {n for _, _, _, n in dc.SWEEPS}
    state, na, nn, rows = dc.sweep_oracle(table, a3, ok, 0, 7, 20, 4097)
    assert set(state.tolist()) == {0, 1, 2}
    assert rows[4096] > 0 and rows[0] > 0 and (rows == 0).any() and na.max() >= 1 and nn.max() >= 1
    # truncating division would count these: a start within a grain before t_begin, an end within one after
    assert ((ts < 0) & (ts > -7) & (te <= 20)).any() and ((ts >= 0) & (te > 20) & (te < 27)).any()
    _, na0, nn0, rows0 = dc.sweep_oracle(table, a3, ok, 0, 7, 0, 4097)
    assert rows0.sum() >= 25 and (na0 + nn0).sum() >= 15
    for t_begin, grain, window, n_win in dc.SWEEPS:                     # traces before t_begin and past the last window
        assert (ts < t_begin).any() and (ts > t_begin + n_win * grain + window).any()
    table, a3, ok = dc.sweep_big_table()
    assert sorted(np.bincount(table.trace).tolist()) == [3, 65_536, 65_537] and 131_000 < table.n_spans < 131_200
    seen = set()
    for sw in dc.BIG_SWEEPS:
        state, na, nn, rows = dc.sweep_oracle(table, a3, ok, *sw)
        seen |= set(rows.tolist())
    assert {0, 65_536, 65_537, 65_536 + 65_537 + 3} <= seen and state[0] == 2 and state[2] == 1
