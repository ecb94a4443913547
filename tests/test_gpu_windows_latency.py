"""GPU checks of mr_windows_latency (csrc/mr_latency.hip): many windows' latency evidence from one
sort, each window's partition its own detector's.  The expected partitions come from mr_detect on the
same tables (an existing, tested entry); values are compared float.hex for float.hex with the numpy
oracle of tests/latency_cases.py and bytewise with mr_op_latency."""
import ctypes as C

import numpy as np
import pytest

import latency_cases as lc
from latency_cases import MIN5, QS

pytestmark = pytest.mark.gpu


def _detect(ctx, dev, t0, t1, a3, ok):
    """mr_detect's state[] (None for an empty window)."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    st = np.zeros(dev.table.n_traces, np.uint8)
    na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
    rc = _lib.load().mr_detect(ctx.h, dev.h, t0, t1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), ptr(st, C.c_uint8),
                               C.byref(na), C.byref(nn), C.byref(nin))
    if rc == _lib.MR_ERR_VALUE and nin.value == 0:
        return None
    ctx.check(rc, "mr_detect")
    return st


def _call(ctx, wins, ops, k, what=1, qs=QS, method=0):
    """(out[n, k, 2, n_q], count[n, k, 2], status[n]) of one raw mr_windows_latency call."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    n = len(wins)
    qv = np.asarray(qs, np.float64)
    spans = (_lib.P * n)(*[w[0].h for w in wins])
    t0 = np.array([w[1] for w in wins], np.int64)
    t1 = np.array([w[2] for w in wins], np.int64)
    a3 = (C.c_void_p * n)(*[w[3].ctypes.data for w in wins])
    ok = (C.c_void_p * n)(*[w[4].ctypes.data for w in wins])
    kk = k if 1 <= k <= 64 else 64            # (the buffers of a call that must fail on k)
    cod = np.full((n, kk), 123456, np.int32)  # entries j >= n_ops[i] are ignored, whatever they hold
    n_ops = np.array([len(o) for o in ops], np.int32)
    for i, o in enumerate(ops):
        cod[i, :min(len(o), kk)] = np.asarray(o)[:kk]
    out = np.full((n, kk, 2, qv.size), -7.0)
    cnt = np.full((n, kk, 2), -7, np.int64)
    status = np.full(n, -7, np.int32)
    ctx.check(_lib.load().mr_windows_latency(ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok,
                                             ptr(cod, C.c_int32), ptr(n_ops, C.c_int32), k, what, ptr(qv, C.c_double),
                                             qv.size, method, ptr(out, C.c_double), ptr(cnt, C.c_int64),
                                             ptr(status, C.c_int32)), "mr_windows_latency")
    return out, cnt, status


@pytest.fixture(scope="module")
def six():
    """Six windows: four 5-minute cuts of one 20-minute table, the no-abnormal-trace table's window,
    an empty window; their top lists from ONE rank_windows call."""
    from microrank_amd import _lib, synth
    from microrank_amd.online_rca import rank_windows
    from microrank_amd.preprocess_data import DeviceSpans

    ctx = _lib.default_context()
    topo, normal, abnormal = synth.window_pair(40, 2000, 3, minutes=20)
    a3, ok, _, _, _ = lc.slo_and_state(normal, abnormal)
    qt, qn, qa = lc.quiet_case()
    qa3, qok, qstate, _, _ = lc.slo_and_state(qn, qa)
    assert (qstate == 2).sum() == 0
    dev, qdev = DeviceSpans(ctx, abnormal), DeviceSpans(ctx, qa)
    b = int(abnormal.tstart.min())
    wins = [(dev, b + i * MIN5, b + (i + 1) * MIN5, a3, ok) for i in range(4)]
    qb = int(qa.tstart.min())
    wins.append((qdev, qb, int(qa.tend.max()), qa3, qok))
    wins.append((dev, 0, 1, a3, ok))   # no trace in [0, 1] ns
    ranked = rank_windows(ctx, wins)
    yield ctx, wins, ranked
    dev.close()
    qdev.close()


def _ops_of(wins, ranked):
    # a window that ranks nothing (no abnormal trace; the empty one) has no top list: ask its table's
    # five most frequent pod-ops instead
    return [r[0] if len(r[0]) else np.argsort(-np.bincount(w[0].table.podop), kind="stable")[:5].astype(np.int32)
            for w, r in zip(wins, ranked)]


def test_six_windows_in_one_call(six):
    from microrank_amd import _lib

    ctx, wins, ranked = six
    assert [r[5] for r in ranked] == [0, 0, 0, 0, 0, _lib.MR_ERR_VALUE]
    assert sum(len(r[0]) > 0 for r in ranked[:4]) >= 2, "the fault should trigger several cuts"
    ops = _ops_of(wins, ranked)
    k = 11
    for what, wname in ((1, "self"), (0, "duration")):
        out, cnt, status = _call(ctx, wins, ops, k, what)
        assert status.tolist() == [0, 0, 0, 0, 0, _lib.MR_ERR_VALUE]
        for i, w in enumerate(wins):
            n = len(ops[i])
            assert not out[i, n:].any() and not cnt[i, n:].any()      # entries j >= n_ops[i] are zeros
            st = _detect(ctx, w[0], w[1], w[2], w[3], w[4])
            if st is None:
                assert i == 5 and not out[i].any() and not cnt[i].any()   # the empty window: zeros
                continue
            rc, o1, c1 = lc.op_latency_call(ctx, w[0], st, ops[i], what, QS, 0, w[1], w[2])
            assert rc == _lib.MR_OK
            assert out[i, :n].tobytes() == o1.tobytes() and cnt[i, :n].tobytes() == c1.tobytes(), (wname, i)
            eo, ec = lc.latency_oracle(w[0].table, st, w[1], w[2], ops[i], wname, QS, "linear")
            assert lc.hexes(out[i, :n]) == lc.hexes(eo) and cnt[i, :n].tolist() == ec.tolist(), (wname, i)
        assert not cnt[4, :, 1].any() and cnt[4, :5, 0].min() > 0   # no abnormal trace: abnormal counts 0


def test_place_independence_and_determinism(six):
    ctx, wins, ranked = six
    ops = _ops_of(wins, ranked)
    out, cnt, status = _call(ctx, wins, ops, 11)
    out2, cnt2, status2 = _call(ctx, wins, ops, 11)
    assert out.tobytes() == out2.tobytes() and cnt.tobytes() == cnt2.tobytes() and status.tolist() == status2.tolist()
    ro, rc, rs = _call(ctx, wins[::-1], ops[::-1], 11)
    assert ro[::-1].tobytes() == out.tobytes() and rc[::-1].tobytes() == cnt.tobytes()
    assert rs[::-1].tolist() == status.tolist()
    for i in (1, 4, 5):   # a window alone gives the same bytes as inside the call
        o1, c1, s1 = _call(ctx, wins[i:i + 1], ops[i:i + 1], 11)
        assert o1[0].tobytes() == out[i].tobytes() and c1[0].tobytes() == cnt[i].tobytes() and s1[0] == status[i]


def test_ranking_unchanged_and_python_layer(six):
    from microrank_amd.online_rca import rank_windows, windows_latency

    ctx, wins, ranked = six
    lat = windows_latency(ctx, wins, [r[0] for r in ranked], q=QS)
    again = rank_windows(ctx, wins)
    for a, b in zip(ranked, again):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]
    out, cnt, _ = _call(ctx, wins, [r[0] for r in ranked], 11)
    for i, r in enumerate(ranked):
        assert list(lat[i]) == [int(c) for c in r[0]]
        for j, c in enumerate(r[0]):
            nrm, abn, n_n, n_a = lat[i][int(c)]
            assert nrm.tobytes() == out[i, j, 0].tobytes() and abn.tobytes() == out[i, j, 1].tobytes()
            assert (n_n, n_a) == (cnt[i, j, 0], cnt[i, j, 1])


def test_argument_errors(six):
    from microrank_amd import _lib

    ctx, wins, ranked = six
    ops = _ops_of(wins, ranked)
    for bad in (dict(k=0), dict(k=65), dict(what=2), dict(method=5), dict(qs=[1.5]), dict(qs=[0.5] * 17)):
        kw = dict(k=11)
        kw.update(bad)
        with pytest.raises(ValueError):
            _call(ctx, wins, ops, **kw)
    with pytest.raises(ValueError):                      # n_ops[i] outside 0..K
        _call(ctx, wins, [np.arange(12)] + ops[1:], 11)
    with pytest.raises(ValueError):                      # an asked op outside [0, n_podops)
        _call(ctx, wins, [np.array([0, 40])] + ops[1:], 11)
    out, cnt, status = _call(ctx, wins, ops, 11)         # the context still answers
    assert status[:5].tolist() == [0] * 5 and cnt.sum() > 0
