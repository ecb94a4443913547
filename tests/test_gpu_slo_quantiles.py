"""GPU checks of mr_slo_quantiles (K4's percentile form, csrc/mr_quantile.hip) and its Python
surface.  Every value is compared bit for bit (float.hex) with np.quantile(durations_of_op, q,
method=...) computed here on the int64 column: no tolerance, no excluded case."""
import contextlib
import ctypes as C
import io

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden, regen_window

pytestmark = pytest.mark.gpu

METHODS = {"linear": 0, "lower": 1, "higher": 2}
QS = [0, 0.25, 1 / 3, 0.5, 0.9, 0.99, 0.999, 1]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


def _table(svcop, dur, n_ops, tstart=None, tend=None):
    """A SpanTable of the given service-op codes and durations (four rows per trace, no parents)."""
    from microrank_amd.spans import SpanTable

    S = len(svcop)
    code = np.asarray(svcop, np.int32)
    names = [f"svc_op{o:04d}" for o in range(n_ops)]
    i64 = lambda a: None if a is None else np.asarray(a, np.int64)
    return SpanTable((np.arange(S) // 4).astype(np.int32), code, code.copy(), np.arange(S, dtype=np.int64),
                     np.full(S, -1, np.int64), np.asarray(dur, np.int64), i64(tstart), i64(tend),
                     [f"t{i:06d}" for i in range((S + 3) // 4)], names, list(names))


def _call(ctx, dev, q, method=0, t0=I64_MIN, t1=I64_MAX, n_q=None):
    """(status, out[n_ops, n_q], count[n_ops]) of one mr_slo_quantiles call."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    qv = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1))
    n = dev.table.n_svcops
    out = np.full((n, max(qv.size, 1)), -7.0)
    cnt = np.full(n, -7, np.int64)
    rc = _lib.load().mr_slo_quantiles(ctx.h, dev.h, t0, t1, ptr(qv, C.c_double), qv.size if n_q is None else n_q,
                                      method, ptr(out, C.c_double), ptr(cnt, C.c_int64))
    return rc, out, cnt


def _last_error(ctx):
    from microrank_amd import _lib

    m = _lib.load().mr_last_error(ctx.h)
    return m.decode() if m else ""


def _check_all(ctx, table, qs, rows=None, t0=I64_MIN, t1=I64_MAX):
    """Upload `table`, run every method and compare with np.quantile over `rows` (default: all)."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    dev = DeviceSpans(ctx, table)
    sel = np.ones(table.n_spans, bool) if rows is None else rows
    per_op = [table.duration[sel & (table.svcop == o)] for o in range(table.n_svcops)]
    counts = None
    for name, code in METHODS.items():
        rc, out, cnt = _call(ctx, dev, qs, code, t0, t1)
        assert rc == _lib.MR_OK, (name, _last_error(ctx))
        assert cnt.tolist() == [a.size for a in per_op], name
        for o, a in enumerate(per_op):
            if a.size == 0:
                assert out[o].tolist() == [0.0] * len(qs), (name, o)
                continue
            exp = np.quantile(a, qs, method=name)
            assert [float(v).hex() for v in out[o]] == [float(v).hex() for v in exp], (name, o, a.size)
        counts = cnt
    dev.close()
    return counts


def test_edge_sizes_lds_sort_path(ctx):
    """Ops of 0 (op 0: a name with no rows), 1, 2, 3, 4, 5, 7, 100, 101 rows interleaved at random;
    S <= 4096 takes the sort's one-block LDS branch.  n = 2 at q = 0.5 takes g >= 0.5; n = 1 and
    q = 1 take the vi >= n - 1 clamp."""
    sizes = [0, 1, 2, 3, 4, 5, 7, 100, 101]
    rng = np.random.default_rng(11)
    op = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(op)
    dur = (rng.lognormal(8.0, 1.5, op.size) + rng.integers(0, 1000, op.size)).astype(np.int64)
    assert op.size <= 4096
    cnt = _check_all(ctx, _table(op, dur, len(sizes)), QS)
    assert cnt.tolist() == sizes and cnt[0] == 0


def _skewed(S, big, seed):
    """300 ops (codes wider than one 8-bit digit) over S rows: op 0 has one row, op 5 `big` rows,
    op 7 fifty rows of one and the same duration, the others a Zipf-like share (at least 1)."""
    n_ops = 300
    rng = np.random.default_rng(seed)
    sizes = np.ones(n_ops, np.int64)
    sizes[5], sizes[7] = big, 50
    rest = S - int(sizes.sum())
    assert rest >= 0
    others = np.array([o for o in range(1, n_ops) if o not in (5, 7)])
    w = 1.0 / (1.0 + np.arange(others.size))
    sizes[others] += rng.multinomial(rest, w / w.sum())
    assert sizes.sum() == S and sizes.min() == 1
    op = np.repeat(np.arange(n_ops), sizes)
    rng.shuffle(op)
    dur = (rng.lognormal(8.0, 1.5, S) + rng.integers(0, 1000, S)).astype(np.int64)
    dur[op == 7] = 12345
    return _table(op, dur, n_ops), sizes


@pytest.mark.parametrize("S,big", [(4097, 1500), (2048 * 9 + 1, 8200), (70_001, 20_000)])
def test_radix_path_and_tile_edges(ctx, S, big):
    """The radix branch at its first size, one key past nine 2048-key tiles, and ~70k rows."""
    table, sizes = _skewed(S, big, S)
    if S > 10_000:
        assert sizes.max() > 8192
    cnt = _check_all(ctx, table, QS)
    assert cnt.tolist() == sizes.tolist()


def test_key_width_negative_minimum(ctx):
    """Durations over [0, 2^40) plus a few negative ones: dmin < 0, a 41-bit duration field beside
    the op bits (a multi-pass sort), a[] restored from the keys."""
    rng = np.random.default_rng(5)
    sizes = [1, 2, 3, 9, 64, 65, 500, 1000, 3366]
    op = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(op)
    dur = rng.integers(0, 1 << 40, op.size, dtype=np.int64)
    dur[rng.choice(op.size, 7, replace=False)] = [-1, -5, -1000, -123456789, -2, -77, -(1 << 20)]
    assert dur.min() < 0 and op.size == 5010
    _check_all(ctx, _table(op, dur, len(sizes)), QS)


def test_key_width_too_wide_is_an_argument_error(ctx):
    """Durations {0, 2^62} with 1000 ops need 63 + 10 key bits: MR_ERR_ARG naming the range."""
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    op = np.repeat(np.arange(1000), 2)
    dur = np.tile(np.array([0, 1 << 62], np.int64), 1000)
    dev = DeviceSpans(ctx, _table(op, dur, 1000))
    rc, out, cnt = _call(ctx, dev, [0.5])
    assert rc == _lib.MR_ERR_ARG
    assert "range" in _last_error(ctx)
    with pytest.raises(ValueError, match="range"):
        ctx.check(rc, "mr_slo_quantiles")
    dev.close()


def _banded():
    """Three bands of rows around the window [10_000, 20_000]; ops 10 and 11 only outside it."""
    rng = np.random.default_rng(3)
    t0, t1 = 10_000, 20_000
    n = 900
    op = rng.integers(0, 10, 3 * n)
    ts = np.concatenate([rng.integers(1_000, 5_000, n), rng.integers(t0, 15_000, n), rng.integers(20_001, 30_000, n)])
    te = np.concatenate([ts[:n] + rng.integers(0, 4_999, n), ts[n:2 * n] + rng.integers(0, 5_000, n),
                         ts[2 * n:] + rng.integers(0, 5_000, n)])
    # rows exactly on each bound (inside), and rows one tick over each bound (outside)
    ts[n:n + 4], te[n:n + 4] = [t0, t0, 15_000, t0], [t0, t1, t1, 12_000]
    ts[n + 4:n + 8], te[n + 4:n + 8] = [t0 - 1, 15_000, t0 - 1, t0], [15_000, t1 + 1, t1 + 1, t1 + 1]
    op[:40], op[2 * n:2 * n + 40] = 10, 11
    op[n + 4:n + 8] = [10, 11, 10, 11]
    dur = (rng.lognormal(8.0, 1.5, 3 * n) + rng.integers(0, 1000, 3 * n)).astype(np.int64)
    order = rng.permutation(3 * n)
    return op[order], dur[order], ts[order], te[order], t0, t1


def test_window(ctx):
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    op, dur, ts, te, t0, t1 = _banded()
    inside = (ts >= t0) & (te <= t1)
    assert ((ts == t0) & inside).any() and ((te == t1) & inside).any()
    assert ((ts == t0 - 1) & (te <= t1)).any() and ((te == t1 + 1) & (ts >= t0)).any()
    table = _table(op, dur, 12, ts, te)
    cnt = _check_all(ctx, table, QS, rows=inside, t0=t0, t1=t1)
    assert cnt[10] == 0 and cnt[11] == 0 and cnt[:10].min() > 0 and cnt.sum() == inside.sum() < op.size
    _check_all(ctx, table, QS)   # the whole table of the same upload data
    # a window that selects nothing
    dev = DeviceSpans(ctx, table)
    rc, out, cnt = _call(ctx, dev, QS, 0, 0, 10)
    assert rc == _lib.MR_OK and not cnt.any() and not out.any()
    dev.close()
    # no trace-level times: a window is a state error, the whole table works
    bare = _table(op, dur, 12)
    dev = DeviceSpans(ctx, bare)
    rc, _, _ = _call(ctx, dev, QS, 0, t0, t1)
    assert rc == _lib.MR_ERR_STATE
    dev.close()
    _check_all(ctx, bare, QS)
    # S = 0
    empty = _table(np.zeros(0, np.int32), np.zeros(0, np.int64), 3)
    for times in (None, np.zeros(0, np.int64)):
        empty.tstart = empty.tend = times
        dev = DeviceSpans(ctx, empty)
        rc, out, cnt = _call(ctx, dev, QS)
        assert rc == _lib.MR_OK and cnt.tolist() == [0, 0, 0] and not out.any()
        dev.close()


def test_argument_errors_leave_the_context_usable(ctx):
    from microrank_amd import _lib
    from microrank_amd._lib import ptr
    from microrank_amd.preprocess_data import DeviceSpans

    rng = np.random.default_rng(9)
    op = rng.integers(0, 5, 600)
    dur = rng.integers(1, 10_000, 600)
    table = _table(op, dur, 5)
    dev = DeviceSpans(ctx, table)
    for q in ([-0.1], [1.5], [float("nan")], [0.5, 1.5], [0.5, float("nan")]):
        rc, _, _ = _call(ctx, dev, q)
        assert rc == _lib.MR_ERR_ARG, q
    assert _call(ctx, dev, [0.5], n_q=0)[0] == _lib.MR_ERR_ARG
    assert _call(ctx, dev, [0.5], n_q=-1)[0] == _lib.MR_ERR_ARG
    assert _call(ctx, dev, [0.5], method=7)[0] == _lib.MR_ERR_ARG
    assert _call(ctx, dev, [0.5], method=-1)[0] == _lib.MR_ERR_ARG
    lib, q1 = _lib.load(), np.array([0.5])
    out, cnt = np.zeros(5), np.zeros(5, np.int64)
    args = lambda **kw: [kw.get("c", ctx.h), kw.get("s", dev.h), I64_MIN, I64_MAX, kw.get("q", ptr(q1, C.c_double)), 1,
                         0, kw.get("out", ptr(out, C.c_double)), kw.get("cnt", ptr(cnt, C.c_int64))]
    for bad in ({"s": None}, {"q": None}, {"out": None}, {"cnt": None}):
        assert lib.mr_slo_quantiles(*args(**bad)) == _lib.MR_ERR_ARG, bad
    assert lib.mr_slo_quantiles(*args(c=None)) == _lib.MR_ERR_ARG
    other = _lib.Context(0)   # a table of another context
    assert lib.mr_slo_quantiles(*args(c=other.h)) == _lib.MR_ERR_ARG
    other.close()
    # the context still works
    rc, out, cnt = _call(ctx, dev, [0.5, 0.99])
    assert rc == _lib.MR_OK
    for o in range(5):
        exp = np.quantile(table.duration[table.svcop == o], [0.5, 0.99])
        assert [float(v).hex() for v in out[o]] == [float(v).hex() for v in exp]
    dev.close()


def test_python_layer():
    """On the committed case `pods_dup_broken` (checked on the CPU: no trace of its abnormal frame
    has max(duration)/1000 exactly equal to its p99 expectation, so the partition does not hang on
    a float tie; pandas' grouped quantile and np.quantile agree bit for bit on it after rounding)."""
    from microrank_amd.anormaly_detector import get_slo, system_anomaly_detect
    from microrank_amd.preprocess_data import get_operation_quantiles, get_operation_slo, get_service_operation_list
    from microrank_amd.spans import _as_ns

    case = load_golden("pods_dup_broken.json")
    ndf, adf = regen_window(case)
    df = ndf.copy()
    ol = get_service_operation_list(df)
    qs = [0.5, 0.99]
    got = get_operation_quantiles(ol, df, qs)
    plain = get_operation_slo(ol, df)
    # the default SLO is what it was: same dict, same hex (the committed golden)
    assert list(plain) == list(case["slo"])
    assert {k: [float(v[0]).hex(), float(v[1]).hex()] for k, v in plain.items()} == case["slo"]
    assert list(got) == list(plain)
    groups = df.groupby("operation")["duration"]
    pq = np.round(groups.quantile(qs) / 1000, 4)
    for name, d in groups:
        exp = np.round(np.quantile(d.to_numpy(np.int64), qs) / 1000.0, 4)
        assert [float(v).hex() for v in got[name]] == [float(v).hex() for v in exp], name
        assert [float(v).hex() for v in got[name]] == [float(pq[(name, q)]).hex() for q in qs], name
        assert all(isinstance(v, np.float64) for v in got[name])
    # other methods, a window (here: one that holds every row), a scalar q
    lo, hi = df["startTime"].min(), df["endTime"].max()
    for method in ("lower", "higher"):
        g2 = get_operation_quantiles(ol, df, 0.9, method=method, window=(lo, hi))
        for name, d in groups:
            exp = np.round(np.quantile(d.to_numpy(np.int64), 0.9, method=method) / 1000.0, 4)
            assert [float(v).hex() for v in g2[name]] == [float(exp).hex()], (method, name)
    assert get_operation_quantiles(ol[:3], df, 0.5).keys() == set(ol[:3])
    with pytest.raises(ValueError):
        get_operation_quantiles(ol, df, 1.5)
    with pytest.raises(ValueError):
        get_operation_quantiles(ol, df, 0.5, method="nearest")
    # the percentile SLO: [Q, 0.0] pairs
    slo = get_operation_slo(ol, df, quantile=0.99)
    assert list(slo) == list(plain)
    for name, v in slo.items():
        assert len(v) == 2 and float(v[0]).hex() == float(got[name][1]).hex() and float(v[1]).hex() == (0.0).hex()
        assert isinstance(v[0], np.float64) and isinstance(v[1], np.float64)
    slo2 = get_slo(ndf.copy(), quantile=0.99)
    assert {k: [float(x).hex() for x in v] for k, v in slo2.items()} == \
        {k: [float(x).hex() for x in v] for k, v in slo.items()}
    # the unchanged detector on the abnormal frame: abnormal iff max(duration)/1000 > sum over the
    # trace's ops, in sorted op order, of count * Q[op] (mr_detect's header comment)
    det = case["detect"]
    a = adf.copy()
    get_service_operation_list(a)
    ts, te = _as_ns(a["startTime"]), _as_ns(a["endTime"])
    w = a[(ts >= det["start_ns"]) & (te <= det["end_ns"])]
    names = sorted(a["operation"].unique())
    exp_ab, exp_no, ties = [], [], 0
    for tid, grp in w.groupby("traceID"):
        mx = int(grp["duration"].max())
        if mx <= 0:
            continue
        count = grp["operation"].value_counts()
        expect = 0.0
        for name in names:
            if name in count.index and name in slo:
                expect = expect + float(count[name]) * float(slo[name][0] + 3 * slo[name][1])
        real = mx / 1000.0
        ties += real == expect
        (exp_ab if real > expect else exp_no).append(tid)
    assert ties == 0 and exp_ab and exp_no
    with contextlib.redirect_stdout(io.StringIO()):
        flag, ab, no = system_anomaly_detect(adf, start_time=pd.Timestamp(det["start_ns"]),
                                             end_time=pd.Timestamp(det["end_ns"]), slo=slo, operation_list=ol)
    assert flag is True
    assert list(ab) == sorted(exp_ab) and list(no) == sorted(exp_no)


def test_determinism(ctx):
    from microrank_amd import _lib
    from microrank_amd.preprocess_data import DeviceSpans

    table, _ = _skewed(2048 * 9 + 1, 8200, 77)
    dev = DeviceSpans(ctx, table)
    a = _call(ctx, dev, QS)
    b = _call(ctx, dev, QS)
    dev.close()
    assert a[0] == b[0] == _lib.MR_OK
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
