"""GPU checks of mr_op_latency (csrc/mr_latency.hip): per asked pod-op and side of a partition the row
count and np.quantile of the rows' duration or self time, compared float.hex for float.hex with the
numpy oracle of tests/latency_cases.py: no tolerance, no excluded case.  The partitions are random
host-made state arrays, so the detector is no part of these tests."""
import ctypes as C

import numpy as np
import pytest

import latency_cases as lc
from latency_cases import I64_MAX, I64_MIN, QS, check_op_latency, last_error, op_latency_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


def _dev(ctx, table):
    from microrank_amd.preprocess_data import DeviceSpans

    return DeviceSpans(ctx, table)


def test_edge_sizes(ctx):
    """(op, side) counts 0, 1, 2, 3, 5, 100, 101 in ~1,000 rows (the sort's one-block branch), an asked
    op with no row at all, rows of state-0 traces that must not count; all methods, both values."""
    table, state, ops = lc.edge_table()
    dev = _dev(ctx, table)
    cnt = check_op_latency(ctx, dev, table, state, ops)
    assert set(cnt.reshape(-1).tolist()) == lc.EDGE_COUNTS and cnt[0].tolist() == [0, 0]
    dev.close()


def test_radix_branch_64_ops_one_twice(ctx):
    """70,001 rows, 300 pod-ops, 64 asked (the limit) -- op 5 with 20,000 rows, op 7 with 50 rows of one
    single value, op 9 asked twice: more than 4096 selected keys."""
    table, state, sizes = lc.skewed_table()
    ops = np.array([5, 7, 9] + [o for o in range(300) if o not in (5, 7, 9)][:60] + [9], np.int32)
    assert ops.size == 64
    dev = _dev(ctx, table)
    cnt = check_op_latency(ctx, dev, table, state, ops)
    assert cnt.sum() > 4096 and cnt[0].sum() > 8192
    assert cnt[2].tolist() == cnt[63].tolist() and cnt[2].sum() > 0    # the duplicate is answered each time
    rc, out, _ = op_latency_call(ctx, dev, state, ops, 1, QS)
    assert out[2].tobytes() == out[63].tobytes()
    assert set(out[1].reshape(-1).tolist()) == {12345.0}
    dev.close()


def test_negative_self_time(ctx):
    """window_pair(40, 2000, 3, dup=0.01, broken=0.05): duplicated spanIDs and broken traces make self
    time negative -- vmin < 0, the values restored from the keys."""
    topo, normal, abnormal = lc.fault_case(dup=0.01, broken=0.05)
    rng = np.random.default_rng(8)
    state = rng.integers(0, 3, abnormal.n_traces).astype(np.uint8)
    v = lc.values(abnormal, "self")
    neg = np.unique(abnormal.podop[(v < 0) & np.isin(state[abnormal.trace], (1, 2))])
    assert neg.size
    ops = np.unique(np.concatenate([neg[:20], np.arange(10)])).astype(np.int32)
    dev = _dev(ctx, abnormal)
    check_op_latency(ctx, dev, abnormal, state, ops, whats=("self",))
    _, out, _ = op_latency_call(ctx, dev, state, ops, 1, [0.0])
    assert out.min() < 0
    dev.close()


def test_window(ctx):
    from microrank_amd import _lib

    table, state, t0, t1 = lc.banded_table()
    ops = np.arange(12, dtype=np.int32)
    dev = _dev(ctx, table)
    cnt = check_op_latency(ctx, dev, table, state, ops, t0=t0, t1=t1)   # rows on a bound count, one tick over do not
    assert cnt[10].sum() == 0 and cnt[11].sum() == 0 and cnt[:10].sum(axis=1).min() > 0
    check_op_latency(ctx, dev, table, state, ops)                       # the whole table of the same upload
    rc, out, cnt = op_latency_call(ctx, dev, state, ops, 1, QS, 0, 0, 10)   # a window that selects nothing
    assert rc == _lib.MR_OK and not cnt.any() and not out.any()
    dev.close()
    bare, state, _, _ = lc.banded_table(times=False)                    # no trace-level times
    dev = _dev(ctx, bare)
    assert op_latency_call(ctx, dev, state, ops, 1, QS, 0, t0, t1)[0] == _lib.MR_ERR_STATE
    check_op_latency(ctx, dev, bare, state, ops)
    dev.close()
    empty = bare.take(np.zeros(0, np.int64))                             # S = 0
    dev = _dev(ctx, empty)
    for what in (0, 1):
        rc, out, cnt = op_latency_call(ctx, dev, state, ops, what, QS)
        assert rc == _lib.MR_OK and not cnt.any() and not out.any()
    dev.close()


def test_key_width_too_wide_is_an_argument_error(ctx):
    """Durations {0, 2^62}: 63 value bits beside the class bits -- MR_ERR_ARG naming the range."""
    from microrank_amd import _lib
    from microrank_amd.spans import SpanTable

    n = 64
    op = np.zeros(n, np.int32)
    dur = np.tile(np.array([0, 1 << 62], np.int64), n // 2)
    table = SpanTable((np.arange(n) // 4).astype(np.int32), op, op.copy(), np.arange(n, dtype=np.int64),
                      np.full(n, -1, np.int64), dur, None, None, [f"t{i}" for i in range(n // 4)], ["p"], ["p"])
    dev = _dev(ctx, table)
    rc, _, _ = op_latency_call(ctx, dev, np.ones(n // 4, np.uint8), [0, 0, 0], 0, [0.5])
    assert rc == _lib.MR_ERR_ARG and "range" in last_error(ctx)
    with pytest.raises(ValueError, match="range"):
        ctx.check(rc, "mr_op_latency")
    dev.close()


def test_argument_errors_leave_the_context_usable(ctx):
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    table, state, ops = lc.edge_table()
    dev = _dev(ctx, table)
    E = _lib.MR_ERR_ARG
    for q in ([-0.1], [1.5], [float("nan")], [0.5, 1.5], [0.5, float("nan")]):
        assert op_latency_call(ctx, dev, state, ops, 1, q)[0] == E, q
    for n_q in (0, -1, 17):
        assert op_latency_call(ctx, dev, state, ops, 1, [0.5] * 17, n_q=n_q)[0] == E, n_q
    assert op_latency_call(ctx, dev, state, ops, 1, [0.5] * 16)[0] == _lib.MR_OK
    for n_ops in (0, -1, 65):
        assert op_latency_call(ctx, dev, state, np.zeros(65, np.int32), 1, [0.5], n_ops=n_ops)[0] == E, n_ops
    for what in (-1, 2):
        assert op_latency_call(ctx, dev, state, ops, what, [0.5])[0] == E
    for method in (-1, 3, 7):
        assert op_latency_call(ctx, dev, state, ops, 1, [0.5], method)[0] == E
    for bad in ([-1], [table.n_podops], [1, 2, table.n_podops]):
        assert op_latency_call(ctx, dev, state, bad, 1, [0.5])[0] == E, bad
    lib, q1, cod = _lib.load(), np.array([0.5]), np.array([1, 2], np.int32)
    out, cnt = np.zeros(4), np.zeros(4, np.int64)
    args = lambda **kw: [kw.get("c", ctx.h), kw.get("s", dev.h), I64_MIN, I64_MAX, kw.get("st", ptr(state, C.c_uint8)),
                         kw.get("ops", ptr(cod, C.c_int32)), 2, 1, kw.get("q", ptr(q1, C.c_double)), 1, 0,
                         kw.get("out", ptr(out, C.c_double)), kw.get("cnt", ptr(cnt, C.c_int64))]
    for bad in ({"s": None}, {"st": None}, {"ops": None}, {"q": None}, {"out": None}, {"cnt": None}, {"c": None}):
        assert lib.mr_op_latency(*args(**bad)) == E, bad
    other = _lib.Context(0)   # a table of another context
    assert lib.mr_op_latency(*args(c=other.h)) == E
    other.close()
    check_op_latency(ctx, dev, table, state, ops, methods=("linear",))   # the context still works
    dev.close()


def test_csum_cache_leaves_the_table_as_it_was(ctx):
    """A second MR_LAT_SELF call gives the same bytes; mr_slo_quantiles, mr_detect and one mr_rca_window
    on a table that has answered MR_LAT_SELF are bytewise what they returned before that call."""
    import bench
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    topo, normal, abnormal = lc.fault_case(dup=0.01, broken=0.05)
    a3, ok, state, t0, t1 = lc.slo_and_state(normal, abnormal)
    dev = _dev(ctx, abnormal)
    lib = _lib.load()

    def snapshot():
        qv = np.array([0.5, 0.99])
        qo, qc = np.zeros((abnormal.n_svcops, 2)), np.zeros(abnormal.n_svcops, np.int64)
        ctx.check(lib.mr_slo_quantiles(ctx.h, dev.h, I64_MIN, I64_MAX, ptr(qv, C.c_double), 2, 0, ptr(qo, C.c_double),
                                       ptr(qc, C.c_int64)), "mr_slo_quantiles")
        st = np.zeros(abnormal.n_traces, np.uint8)
        na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
        ctx.check(lib.mr_detect(ctx.h, dev.h, t0, t1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), ptr(st, C.c_uint8),
                                C.byref(na), C.byref(nn), C.byref(nin)), "mr_detect")
        e, codes, scores, wna, wnn = bench.run_window(ctx, dev, t0, t1, a3, ok, _lib.MR_FP64)
        return (qo.tobytes(), qc.tobytes(), st.tobytes(), na.value, nn.value, nin.value, e, np.asarray(codes).tobytes(),
                np.asarray(scores).tobytes(), wna, wnn), st

    before, st = snapshot()
    assert st.tolist() == state.tolist()          # mr_detect's partition is the oracle's
    ops = np.arange(12, dtype=np.int32)
    a = op_latency_call(ctx, dev, st, ops, 1, QS)
    b = op_latency_call(ctx, dev, st, ops, 1, QS)
    assert a[0] == b[0] == _lib.MR_OK
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    eo, ec = lc.latency_oracle(abnormal, st, I64_MIN, I64_MAX, ops, "self", QS, "linear")
    assert lc.hexes(a[1]) == lc.hexes(eo) and a[2].tolist() == ec.tolist()
    after, _ = snapshot()
    assert before == after
    dev.close()


def test_shard_table(ctx):
    """A shard of a larger table (row given): MR_LAT_SELF is a state error -- children may lie on
    another rank -- and MR_LAT_DURATION answers."""
    from microrank_amd import _lib

    table, state, ops = lc.edge_table()
    sub = table.shard(0, 2)
    dev = _dev(ctx, sub)
    assert op_latency_call(ctx, dev, state, ops, 1, QS)[0] == _lib.MR_ERR_STATE
    check_op_latency(ctx, dev, sub, state, ops, whats=("duration",))
    dev.close()
