"""Exemplar traces of a window batch on the GPU: mr_windows_batch_exemplars through
rank_windows(..., exemplars=m), sweep_rank and the driver.

Windows and their oracle side: window_exemplar_cases (their properties are asserted on the CPU by
test_window_exemplar_cases).  Five small windows reach: a full wave tile plus a tile of one trace, one
trace alone, several tiles with a ragged last one, a thousand traces with a few distinct scores (exact
ties inside and at the m = 32 cut), and a table whose times vary within a trace (the per-span-time
build: a graph with a trace-major incidence, answered through mr_graph_exemplars' kernels).

Bounds: a returned score against the oracle's r_K of the same trace 1e-10 relative (fp64, 25
iterations) / 1e-4 (fp32, 7 iterations) -- test_gpu_exemplars' RTOL64 / RTOL32.  Trace identity is
claimed only where the oracle separates: ties and near-ties (within the bound) may resolve either way.
Between the layout-order build and the general builds scores agree to 1e-9 relative (the builds order
their sums differently, about 1e-12), lists wherever the oracle separates neighbours by more than 1e-8.
"""
import contextlib
import ctypes as C
import csv
import io
import os

import numpy as np
import pytest

import window_exemplar_cases as wc
from conftest import load_golden

pytestmark = pytest.mark.gpu

RTOL = {"fp64": 1e-10, "fp32": 1e-4}
ROUTE_RTOL, ROUTE_SEP = 1e-9, 1e-8
MS = (1, 4, 32)
KNOBS = ("MR_EX_BLOCKS", "MR_WIN_GROUP", "MR_WIN_CHUNK", "MR_TR_MERGE", "MR_NO_LO", "MR_NO_LO_WIN", "MR_NO_INDEX",
         "MR_KIND_TEST_COLLIDE")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


def _upload(ctx, env):
    from microrank_amd.anormaly_detector import slo_arrays
    from microrank_amd.preprocess_data import DeviceSpans

    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        devs = {n: DeviceSpans(ctx, wc.table(n)[0]) for n in wc.NAMES}
    wins = {}
    for n in wc.NAMES:
        st, slo, _, t0, t1 = wc.table(n)
        a3, ok = slo_arrays(st, slo)
        wins[n] = (devs[n], t0, t1, a3, ok)
    return devs, wins


@pytest.fixture(scope="module")
def wins(ctx):
    """name -> (DeviceSpans, t0, t1, a3, ok)."""
    devs, w = _upload(ctx, {})
    yield w
    for d in devs.values():
        d.close()


@pytest.fixture(scope="module")
def wins_no_lo(ctx):
    """The same windows on tables uploaded without their layout order (MR_NO_LO)."""
    devs, w = _upload(ctx, {"MR_NO_LO": "1"})
    yield w
    for d in devs.values():
        d.close()


def _rank(ctx, ws, m=None, precision="fp64", **kw):
    from microrank_amd.online_rca import rank_windows

    kw.setdefault("iters", wc.ITERS[precision])
    return rank_windows(ctx, ws, precision=precision, exemplars=m, **kw)


def _bits(res):
    """A window's tuple as comparable bytes: the six plain elements, then the exemplar rows."""
    six = (res[0].tobytes(), res[1].tobytes()) + tuple(res[2:6])
    if len(res) == 6:
        return six
    return six + (tuple((c, tuple((t, s.tobytes()) for t, s in lst)) for c, lst in res[6].items()),)


def _check(name, res, m, precision, plain=None):
    """One window's answer against the oracle (section 1 of the issue's list)."""
    from microrank_amd import _lib

    K, rtol = wc.ITERS[precision], RTOL[precision]
    o = wc.oracle(name, K)
    abnormal = set(wc.detected(name)[0])
    pairs = wc.span_pairs(name)
    assert len(res) == 7 and res[5] == _lib.MR_OK and (res[2], res[3]) == (o.n_abnormal, o.n_normal)
    if plain is not None:
        assert _bits(res)[:6] == _bits(plain), f"{name}: the keyword changed the ranking"
    codes, ex = res[0].tolist(), res[6]
    assert list(ex) == codes and len(codes) == wc.K_TOP
    if precision == "fp64":
        assert codes == o.top
    worst = 0.0
    for code in codes:
        lst, what = ex[code], f"{name} {precision} m={m} pod-op {code}"
        row = o.rows.get(code)
        if row is None:   # only normal traces hold it: no node of the abnormal traces' graph
            assert lst == [], what
            continue
        cov = len(row)
        n = min(m, cov)
        assert len(lst) == n, f"{what}: {len(lst)} exemplars, coverage {cov}"
        tr = np.array([t for t, _ in lst], np.int64)
        sc = np.array([s for _, s in lst], np.float64)
        assert all(isinstance(s, np.float64) for _, s in lst) and len(set(tr.tolist())) == n
        assert all(t in abnormal and (t, code) in pairs for t in tr.tolist()), what
        assert (np.diff(sc) <= 0).all(), what
        same = np.flatnonzero(sc[1:].view(np.uint64) == sc[:-1].view(np.uint64))
        assert (tr[same + 1] > tr[same]).all(), f"{what}: equal scores not in trace code order"
        gi = np.minimum(np.searchsorted(o.trace_codes, tr), o.trace_codes.size - 1)
        assert (o.trace_codes[gi] == tr).all() and np.isin(gi, row).all(), what
        ref_own = o.r[gi]
        best = np.sort(o.r[row])[::-1]
        err = max(np.max(np.abs(sc - ref_own) / ref_own), np.max(np.abs(sc - best[:n]) / best[:n]))
        worst = max(worst, float(err))
        np.testing.assert_allclose(sc, ref_own, rtol=rtol, atol=0, err_msg=what)
        np.testing.assert_allclose(sc, best[:n], rtol=rtol, atol=0, err_msg=what)
        rest = np.setdiff1d(row, gi)
        if rest.size:
            assert o.r[rest].max() <= sc[-1] * (1 + rtol), f"{what}: a better trace was left out"
        if n == cov:
            assert set(gi.tolist()) == set(row.tolist()), what
    print(f"{name} {precision} m={m}: max rel diff vs the oracle {worst:.3e}")


# ---------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_against_oracle(ctx, wins, precision, m):
    every = [wins[n] for n in wc.NAMES]
    plain = _rank(ctx, every, None, precision)
    batch = _rank(ctx, every, m, precision)
    for n, res, p in zip(wc.NAMES, batch, plain):
        _check(n, res, m, precision, p)
    for n in wc.NAMES:
        (alone,) = _rank(ctx, [wins[n]], m, precision)
        _check(n, alone, m, precision, _rank(ctx, [wins[n]], None, precision)[0])
    assert any(lst == [] for lst in batch[wc.NAMES.index("one_trace")][6].values())


def _raw(ctx, ws, m, top_max=5, fill=7):
    """mr_windows_batch_exemplars itself, its output arrays pre-filled with `fill`."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    n, k = len(ws), top_max + 6
    spans = (_lib.P * n)(*[w[0].h for w in ws])
    t0, t1 = np.array([w[1] for w in ws], np.int64), np.array([w[2] for w in ws], np.int64)
    a3 = (C.c_void_p * n)(*[w[3].ctypes.data for w in ws])
    ok = (C.c_void_p * n)(*[w[4].ctypes.data for w in ws])
    codes, scores = np.zeros(n * k, np.int32), np.zeros(n * k)
    n_out, na, nn, status = (np.zeros(n, np.int32) for _ in range(4))
    edges = np.zeros(n, np.int64)
    nm = n * k * max(m, 1)
    ex_t, ex_s, ex_c = np.full(nm, fill, np.int32), np.full(nm, float(fill)), np.full(n * k, fill, np.int32)
    rc = _lib.load().mr_windows_batch_exemplars(
        ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok, 0, top_max, _lib.MR_FP64, ptr(codes, C.c_int32),
        ptr(scores, C.c_double), ptr(n_out, C.c_int32), ptr(edges, C.c_int64), ptr(na, C.c_int32), ptr(nn, C.c_int32),
        ptr(status, C.c_int32), 25, 0.0, 1, None, None, m, ptr(ex_t, C.c_int32), ptr(ex_s, C.c_double), ptr(ex_c, C.c_int32))
    return rc, n_out, ex_t.reshape(n, k, -1), ex_s.reshape(n, k, -1), ex_c.reshape(n, k)


def test_padding_and_argument_errors(ctx, wins):
    from microrank_amd import _lib

    ws = [wins["ragged"], wins["one_trace"]]
    rc, n_out, tr, sc, cnt = _raw(ctx, ws, 32)
    assert rc == _lib.MR_OK and n_out.tolist() == [wc.K_TOP] * 2
    for i, name in enumerate(("ragged", "one_trace")):
        cov = list(wc.coverage(name).values())
        assert cnt[i].tolist() == [min(32, c) for c in cov]
        for j, c in enumerate(cnt[i]):
            assert (tr[i, j, :c] >= 0).all() and (sc[i, j, :c] > 0).all()
            assert (tr[i, j, c:] == -1).all() and (sc[i, j, c:] == 0.0).all() and not np.signbit(sc[i, j, c:]).any()
    assert (cnt < 32).any() and (cnt == 32).any() and (cnt == 0).any()
    for m in (0, 33, -1):
        assert _raw(ctx, ws, m)[0] == _lib.MR_ERR_ARG, m
    assert _raw(ctx, ws, 4, top_max=59)[0] == _lib.MR_ERR_ARG   # top_max + 6 > 64 ops
    assert _lib.load().mr_windows_batch_exemplars(ctx.h, 0, None, None, None, None, None, 0, 5, _lib.MR_FP64, None, None, None,
                                                  None, None, None, None, 25, 0.0, 1, None, None, 4, None, None,
                                                  None) == _lib.MR_ERR_ARG


# ---------------------------------------------------------------------------- 2. prefix and cut invariance
def test_smaller_m_is_a_prefix(ctx, wins):
    every = [wins[n] for n in wc.NAMES]
    full = _rank(ctx, every, 32)
    for m in (1, 4):
        for n, a, b in zip(wc.NAMES, _rank(ctx, every, m), full):
            assert _bits(a)[:6] == _bits(b)[:6]
            assert {c: [(t, s.tobytes()) for t, s in lst] for c, lst in a[6].items()} == \
                   {c: [(t, s.tobytes()) for t, s in lst[:m]] for c, lst in b[6].items()}, (n, m)


@pytest.mark.parametrize("knob,values", [("MR_EX_BLOCKS", ("1", "7")), ("MR_WIN_GROUP", ("1",)), ("MR_WIN_CHUNK", ("1",))])
def test_cuts_do_not_change_the_answer(ctx, wins, monkeypatch, knob, values):
    every = [wins[n] for n in wc.NAMES]
    want = [_bits(r) for r in _rank(ctx, every, 32)]
    assert any(r[6] for r in want)
    for v in values:
        monkeypatch.setenv(knob, v)
        assert [_bits(r) for r in _rank(ctx, every, 32)] == want, (knob, v)


@pytest.mark.parametrize("name", wc.NAMES)
def test_position_in_the_call(ctx, wins, name):
    (alone,) = _rank(ctx, [wins[name]], 32)
    others = [wins[n] for n in wc.NAMES if n != name][:3]
    five = _rank(ctx, [wins[name]] + others + [wins[name]], 32)
    assert _bits(five[0]) == _bits(alone) == _bits(five[4]), name


def test_run_merged_graphs(ctx, wins, monkeypatch):
    """MR_TR_MERGE: 1 (runs walked by their heads) and 2 (the run rotations alone) agree bitwise; both
    hold to the oracle bound that the default (0) holds to."""
    got = {}
    for v in ("0", "1", "2"):
        monkeypatch.setenv("MR_TR_MERGE", v)
        (got[v],) = _rank(ctx, [wins["ties"]], 32)
        _check("ties", got[v], 32, "fp64")
    assert _bits(got["1"]) == _bits(got["2"])
    monkeypatch.delenv("MR_TR_MERGE")
    assert _bits(_rank(ctx, [wins["ties"]], 32)[0]) == _bits(got["0"])


# ---------------------------------------------------------------------------- 3. routes
def _same_answer(name, a, b, m):
    """Two builds' answers: scores to ROUTE_RTOL; the same traces wherever the oracle separates a
    trace from its neighbours (and from the first one left out) by more than ROUTE_SEP relative, else
    the same sets up to members of that near-equal run."""
    o = wc.oracle(name, 25)
    assert a[0].tolist() == b[0].tolist() and a[2:6] == b[2:6]
    np.testing.assert_allclose(b[1], a[1], rtol=ROUTE_RTOL, atol=0)
    for code in a[0].tolist():
        la, lb = a[6][code], b[6][code]
        assert len(la) == len(lb), (name, code)
        if not la:
            continue
        np.testing.assert_allclose([s for _, s in lb], [s for _, s in la], rtol=ROUTE_RTOL, atol=0, err_msg=f"{name} {code}")
        row = o.rows[code]
        val = dict(zip(o.trace_codes[row].tolist(), o.r[row].tolist()))
        for (ta, _), (tb, _) in zip(la, lb):
            if ta != tb:   # a swap inside a near-equal run of the oracle's values
                assert abs(val[ta] - val[tb]) <= ROUTE_SEP * max(val[ta], val[tb]), (name, code, ta, tb)


@pytest.mark.parametrize("name", ["ragged", "mid", "ties"])
def test_routes_agree(ctx, wins, wins_no_lo, monkeypatch, name):
    (base,) = _rank(ctx, [wins[name]], 32)
    (no_lo,) = _rank(ctx, [wins_no_lo[name]], 32)   # a table without a layout order
    _check(name, no_lo, 32, "fp64")
    _same_answer(name, base, no_lo, 32)
    monkeypatch.setenv("MR_NO_LO_WIN", "1")         # the batch's general build on a table that has one
    (no_lo_win,) = _rank(ctx, [wins[name]], 32)
    _check(name, no_lo_win, 32, "fp64")
    _same_answer(name, base, no_lo_win, 32)


# ---------------------------------------------------------------------------- 4. tol
def test_stop_at_tol(ctx, wins):
    every = [wins[n] for n in wc.NAMES]
    info = []
    got = _rank(ctx, every, 5, tol=1e-6, iters=60, check_every=4, info=info)
    assert len(info) == len(every)
    for k in sorted({i["iters"] for i in info}):
        assert 1 <= k < 60
        fixed = _rank(ctx, every, 5, iters=k)
        for n, i, a, b in zip(wc.NAMES, info, got, fixed):
            if i["iters"] == k:
                assert _bits(a) == _bits(b), n
    assert any(r[6] and any(r[6].values()) for r in got)


# ---------------------------------------------------------------------------- 5. nothing ranked
def test_nothing_ranked(ctx, wins):
    from microrank_amd import _lib

    dev, t0, t1, a3, ok = wins["one_trace"]
    ws = [(dev, t0, t1, a3 * 1e6, ok),                      # no trace exceeds it: no abnormal trace
          (dev, t1 + 10**12, t1 + 2 * 10**12, a3, ok),      # an empty window
          (dev, t0, t1, a3 * 1e-6, ok),                     # every trace exceeds it: no normal trace
          wins["one_trace"]]
    plain, got = _rank(ctx, ws), _rank(ctx, ws, 3)
    for p, g in zip(plain, got):
        assert _bits(g)[:6] == _bits(p)
    assert [g[5] for g in got] == [_lib.MR_OK, _lib.MR_ERR_VALUE, _lib.MR_OK, _lib.MR_OK]
    assert got[0][2] == 0 and got[2][3] == 0
    assert got[0][6] == {} and got[1][6] == {} and got[2][6] == {}
    last = got[3][6]
    assert len(last) == wc.K_TOP and [] in last.values() and any(last.values())


# ---------------------------------------------------------------------------- 6. the driver
def _driver(adf, case, **kw):
    from microrank_amd import online_rca

    slo_d = {k: [np.float64(float.fromhex(a)), np.float64(float.fromhex(b))] for k, (a, b) in case["slo"].items()}
    buf = io.StringIO()
    err = None
    try:
        with contextlib.redirect_stdout(buf):
            online_rca.online_anomaly_detect_RCA(adf.copy(), slo_d, case["operation_list"], **kw)
    except TypeError as e:
        err = type(e).__name__
    return buf.getvalue(), err, slo_d


def test_driver_writes_exemplars(ctx, tmp_path, monkeypatch):
    import pandas as pd

    from microrank_amd import _lib, online_rca, synth
    from microrank_amd._lib import ptr

    case = load_golden("stream.json")
    _, adf = synth.stream_dataframes(**case["params"])
    monkeypatch.chdir(tmp_path)
    out0, err0, slo_d = _driver(adf, case)
    assert os.path.exists("result.csv") and not os.path.exists("exemplars.csv")
    csv0 = open("result.csv", "rb").read()
    out3, err3, _ = _driver(adf, case, exemplars=3)
    assert (out3, err3) == (out0, err0) and open("result.csv", "rb").read() == csv0
    rows = list(csv.DictReader(open("exemplars.csv")))
    assert rows and list(rows[0]) == ["result", "rank", "trace", "score"]
    ops = [r["result"] for r in csv.DictReader(open("result.csv"))]
    per = {}
    for r in rows:
        per.setdefault(r["result"], []).append(r)
    assert set(per) <= set(ops)
    for op, rs in per.items():
        assert len(rs) <= 3 and [int(r["rank"]) for r in rs] == list(range(1, len(rs) + 1))
        sc = [float(r["score"]) for r in rs]
        assert sc == sorted(sc, reverse=True) and all(s > 0 for s in sc)
    # the abnormal traces of the last triggered window of the driver's chain
    plan = online_rca._sweep_plan(adf.copy(), slo_d, adf["startTime"].min(), adf["endTime"].max(), pd.Timedelta(minutes=5),
                                  pd.Timedelta(minutes=4), ctx)
    assert plan is not None
    last = [e for e in online_rca.sweep_chain(plan) if e[0] == "window" and e[4]][-1][1]
    t0 = plan["t_begin"] + last * plan["grain"]
    table = plan["table"]
    state = np.zeros(table.n_traces, np.uint8)
    na, nn, nin = C.c_int32(), C.c_int32(), C.c_int64()
    ctx.check(_lib.load().mr_detect(ctx.h, plan["dev"].h, t0, t0 + plan["step_n"] * plan["grain"], ptr(plan["a3"], C.c_double),
                                    ptr(plan["ok"], C.c_uint8), ptr(state, C.c_uint8), C.byref(na), C.byref(nn),
                                    C.byref(nin)), "mr_detect")
    names = table.trace_names
    abnormal = {str(names[t]) if names is not None else str(t) for t in np.flatnonzero(state == 2)}
    assert abnormal and {r["trace"] for r in rows} <= abnormal


def test_driver_window_by_window(ctx, tmp_path, monkeypatch):
    """A frame whose times vary within a trace takes the driver's window-by-window loop: exemplars.csv
    comes from window_exemplars there; stdout and result.csv stay as without the keyword."""
    from microrank_amd import online_rca, synth

    st, slo, _, _, _ = wc.table("span_times")
    n_ops, _, _, _, _ = wc.CASES["span_times"]
    df = synth.to_dataframe(st, synth.make_topology(n_ops, 3))
    assert online_rca._sweep_plan(df.copy(), slo, df["startTime"].min(), df["endTime"].max(), online_rca.RCAStream.WINDOW,
                                  online_rca.RCAStream.STEP_ABNORMAL, ctx) is None
    monkeypatch.chdir(tmp_path)
    out = []
    for kw in ({}, dict(exemplars=2)):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            online_rca.online_anomaly_detect_RCA(df.copy(), slo, list(st.svcop_names), **kw)
        out.append((buf.getvalue(), open("result.csv", "rb").read()))
        assert os.path.exists("exemplars.csv") == bool(kw)
    assert out[0] == out[1]
    rows = list(csv.DictReader(open("exemplars.csv")))
    ops = [r["result"] for r in csv.DictReader(open("result.csv"))]
    assert rows and {r["result"] for r in rows} <= set(ops) and {r["trace"] for r in rows} <= set(st.trace_names)
    assert max(int(r["rank"]) for r in rows) <= 2
