"""GPU check of what the four window-list evidence entries share (csrc/mr_evidence.h): windows_latency,
windows_kind_breakdown, windows_call_edges and windows_timeline over ONE list of windows that mixes an empty
window, two tables, shared SLO array objects, a copy of them at another address, a repeated asked op and
a window that asks nothing.  Each entry's own oracle tests are elsewhere; here every answer is compared,
exactly, with the same entry asked about that window alone."""
import numpy as np
import pytest

import kind_breakdown_cases as kb
import timeline_cases as tc

pytestmark = pytest.mark.gpu

Q, BUCKETS, M = (0.5, 0.99), 30, 8
KNOBS = ("MR_KB_CHUNK", "MR_CE_CHUNK", "MR_TL_CHUNK")


def canon(x):
    """An answer as plain Python values (arrays as lists), for exact comparison."""
    if isinstance(x, dict):
        return {k: canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    return x.tolist() if isinstance(x, (np.ndarray, np.generic)) else x


@pytest.fixture(scope="module")
def front():
    """(ctx, the five windows, their asked ops, (a, b, c)).  Table A is `ragged`, table B `one_trace`: the same
    generator, so the same service-ops, under an SLO constant that leaves ONE abnormal trace where A's leaves
    about half -- B's partition under A's SLO arrays would be another."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    A, B = tc.window("ragged"), tc.window("one_trace")
    assert A.table.n_svcops == B.table.n_svcops and not np.array_equal(A.a3, B.a3)
    assert not np.array_equal(A.state, B.state)
    a, b = kb.top_ops(A.table, A.state, 2)
    c = kb.top_ops(B.table, B.state, 1)[0]
    da, db = DeviceSpans(ctx, A.table), DeviceSpans(ctx, B.table)
    wins = [(da, A.t0 - 1000, A.t0 - 1, A.a3, A.ok),          # (0) empty: before the table's first start
            (da, A.t0, A.t1, A.a3, A.ok),                     # (1) table A, SLO pair X
            (db, B.t0, B.t1, B.a3, B.ok),                     # (2) table B, SLO pair Y
            (da, A.t0, A.t1, A.a3, A.ok),                     # (3) table A, the same array objects X
            (da, A.t0, A.t1, A.a3.copy(), A.ok.copy())]       # (4) table A, a copy of X at another address
    yield ctx, wins, [[a], [a, b, a], [c], [], [b]], (a, b, c)
    da.close()
    db.close()


def entries():
    from microrank_amd import online_rca as o

    return {"latency": lambda ctx, w, ops: o.windows_latency(ctx, w, ops, q=Q, what="self"),
            "kinds": lambda ctx, w, ops: o.windows_kind_breakdown(ctx, w, ops, m=M),
            "calls": lambda ctx, w, ops: o.windows_call_edges(ctx, w, ops, m=M),
            "timeline": lambda ctx, w, ops: o.windows_timeline(ctx, w, ops, buckets=BUCKETS, what="self")}


def empty_answer(name):
    """The documented answer for an asked op of an empty window."""
    zb = [[0, 0]] * BUCKETS
    return {"latency": [[0.0] * len(Q), [0.0] * len(Q), 0, 0],
            "kinds": [[], 0, 0, 0],
            "calls": [[[], 0, [0, 0]], [[], 0, [0, 0]]],
            "timeline": {"cnt": zb, "sum": zb, "max": zb, "out": [[0, 0], [0, 0]]}}[name]


def test_status_vector(front):
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows

    ctx, wins, _, _ = front
    assert [r[5] for r in rank_windows(ctx, wins)] == [_lib.MR_ERR_VALUE, 0, 0, 0, 0]


@pytest.mark.parametrize("chunk", [None, "2"])
@pytest.mark.parametrize("name", ["latency", "kinds", "calls", "timeline"])
def test_window_list(front, name, chunk, monkeypatch):
    ctx, wins, ops, (a, b, c) = front
    fn = entries()[name]
    alone = [canon(fn(ctx, [w], [o])[0]) for w, o in zip(wins, ops)]   # (no knob: a call of one window is one chunk)
    first_a = canon(fn(ctx, [wins[1]], [[a]])[0])[a]
    if chunk is not None:
        for k in KNOBS:
            monkeypatch.setenv(k, chunk)   # (read per call)
    got = canon(fn(ctx, wins, ops))
    zero = got[0][a]
    if name == "timeline":   # (the bucket starts are the grid's, not an answer)
        zero = {k: v for k, v in zero.items() if k != "start"}
    assert zero == empty_answer(name)
    assert got == alone                               # each window's answer is that of the window asked alone
    assert list(got[1]) == [a, b] and got[1][a] == first_a   # the repeated op is answered as its first appearance
    assert got[4][b] == got[1][b]                     # an equal SLO pair at another address: the same partition
    assert list(got[2]) == [c] and got[3] == {}       # nothing asked: nothing answered
