"""The window entries' iteration count, convergence report and stop at a tolerance on the GPU
(mr_windows_batch_ex / mr_rca_window_ex through rank_windows / rca_window and the driver).

Windows (bench.make_window(seed, ops, traces), the SLO of the normal table from mr_slo, the window
[tstart.min(), + 5 min]):
  A = (4242, 300, 2000)  both graphs take the last-block finish (N <= 512);
  B = (4242, 600, 3000)  a ~100-op last-block graph and a 600-op pf graph in one launch;
  C = (77, 300, 2000);
  D = (5, 10000, 3000)   one abnormal trace; the other graph has ~5.5k ops, more than one k_resid block.
The oracle side is tests/test_gpu_rca.py::_oracle_rca with the iteration count as an argument:
s_k = orc.power_iteration(g, v, iters=k), s_0 = ones(N)/(N+T), the residual after K iterations
max|s_K - s_{K-1}|.  Bounds: 1e-10 relative on scores (fp64), 1e-4 (fp32); residuals 2e-10 / 2e-4
absolute (two parity-bounded vectors of maximum 1).  Margins the cases rest on are
asserted on the oracle's values first, so that a drifting generator fails there.
"""
import contextlib
import functools
import io
import os
import types

import numpy as np
import pytest

import oracle as orc
from conftest import load_golden

pytestmark = pytest.mark.gpu

WINDOWS = {"A": (4242, 300, 2000), "B": (4242, 600, 3000), "C": (77, 300, 2000), "D": (5, 10000, 3000)}
ATOL64, ATOL32 = 2e-10, 2e-4
KNOBS = ("MR_WIN_GROUP", "MR_WIN_CHUNK", "MR_TR_PF", "MR_WIN_SPEC_EARLY", "MR_NO_LO", "MR_NO_LO_WIN",
         "MR_KIND_TEST_COLLIDE")


# ---------------------------------------------------------------------------- the windows and their oracle
@functools.lru_cache(maxsize=None)
def table(name):
    import bench

    _, normal, abnormal = bench.make_window(*WINDOWS[name])
    t0 = int(abnormal.tstart.min())
    return normal, abnormal, t0, t0 + 5 * 60 * 10**9


@functools.lru_cache(maxsize=None)
def slo(name):
    import bench
    from microrank_amd import _lib

    a3, ok = bench.slo_from_gpu(_lib.default_context(), table(name)[0])
    a3.setflags(write=False)
    ok.setflags(write=False)
    return a3, ok


@functools.lru_cache(maxsize=None)
def oracle_graphs(name):
    """The detector's lists and the window's two graphs: index 0 the graph of the detector's abnormal
    traces (ranked with anomaly False, T1), 1 the graph of its normal traces (anomaly True)."""
    _, st, t0, t1 = table(name)
    a3, ok = slo(name)
    a3map = {i: float(a3[i]) for i in range(len(a3)) if ok[i]}
    _, ab, no = orc.detect(st.trace, st.svcop, st.duration, st.tstart, st.tend, t0, t1, a3map)
    out = []
    for lst, anomaly in ((ab, False), (no, True)):
        sel = np.zeros(st.n_traces, bool)
        sel[lst] = True
        g = orc.span_graph(st.trace, st.podop, st.span, st.parent, sel).as_graph()
        out.append((g, orc.preference(g, orc.trace_kinds(g), anomaly)))
    return len(ab), len(no), out


@functools.lru_cache(maxsize=None)
def s_k(name, which, k):
    g, v = oracle_graphs(name)[2][which]
    s = np.ones(g.N) / float(g.N + g.T) if k == 0 else orc.power_iteration(g, v, iters=k)
    s.setflags(write=False)
    return s


def oracle_resid(name, k):
    """(residual of the graph ranked as normal, of the one ranked as anomaly) after k iterations."""
    return tuple(float(np.max(np.abs(s_k(name, w, k) - s_k(name, w, k - 1)))) for w in (0, 1))


@functools.lru_cache(maxsize=None)
def oracle_rank(name, k, top_max=5):
    na, nn, gs = oracle_graphs(name)
    res = [orc.weights(gs[w][0], s_k(name, w, k)) for w in (0, 1)]   # [normal, anomaly]
    top, score, _ = orc.spectrum(res[1][0], res[0][0], nn, na, top_max, res[0][1], res[1][1], "dstar2")
    return list(top), np.array(score, np.float64), na, nn


def edges_per_iteration(name):
    return sum(2 * int(g.sr_o.size) + int(g.ss_c.size) for g, _ in oracle_graphs(name)[2])


# ---------------------------------------------------------------------------- the device side
@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


def _upload(ctx, env):
    from microrank_amd.preprocess_data import DeviceSpans

    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        devs = {n: DeviceSpans(ctx, table(n)[1]) for n in WINDOWS}
    return devs


@pytest.fixture(scope="module")
def wins(ctx):
    """name -> (DeviceSpans, t0, t1, a3, ok): the tables with their layout order."""
    devs = _upload(ctx, {})
    yield {n: (devs[n], table(n)[2], table(n)[3]) + slo(n) for n in WINDOWS}
    for d in devs.values():
        d.close()


@pytest.fixture(scope="module")
def wins_general(ctx):
    """The same windows on tables uploaded without their layout order (MR_NO_LO: the general build)."""
    devs = _upload(ctx, {"MR_NO_LO": "1"})
    yield {n: (devs[n], table(n)[2], table(n)[3]) + slo(n) for n in WINDOWS}
    for d in devs.values():
        d.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def rank(ctx, ws, **kw):
    """rank_windows with a report: [(result tuple, report dict)] per window."""
    from microrank_amd.online_rca import rank_windows

    info = []
    got = rank_windows(ctx, ws, info=info, **kw)
    assert len(info) == len(got) == len(ws)
    return list(zip(got, info))


def single(ctx, w, **kw):
    """rca_window on a resident table (codes for names, the SLO handed on as [a3, 0.0]): the same
    (result tuple, report dict) as rank()'s, status 0."""
    from microrank_amd.online_rca import rca_window

    dev, t0, t1, a3, ok = w
    tab = types.SimpleNamespace(n_svcops=len(a3), svcop_names=list(range(len(a3))), podop_names=None)
    slo_d = {i: [float(a3[i]), 0.0] for i in range(len(a3)) if ok[i]}
    info = {}
    r = rca_window(None, t0, t1, slo_d, ctx=ctx, table=tab, dev=dev, info=info, **kw)
    return (np.array(r["top"], np.int32), np.array(r["score"], np.float64), r["n_abnormal"], r["n_normal"], r["edges"],
            0), info


def bits(x):
    return np.float64(x).tobytes()


def assert_same(a, b, what=""):
    """Two (result, report) pairs, bit for bit."""
    (ra, ia), (rb, ib) = a, b
    assert list(ra[0]) == list(rb[0]), what
    assert ra[1].tobytes() == rb[1].tobytes(), what
    assert ra[2:] == rb[2:], what
    assert ia["iters"] == ib["iters"], what
    assert bits(ia["resid_normal"]) == bits(ib["resid_normal"]), (what, ia, ib)
    assert bits(ia["resid_anomaly"]) == bits(ib["resid_anomaly"]), (what, ia, ib)


def check_against_oracle(name, got, k, what):
    (codes, scores, na, nn, edges, status), info = got
    top, score, ona, onn = oracle_rank(name, k)
    print(f"{what} {name} iters={k}: max rel score diff "
          f"{np.max(np.abs(scores - score[:len(scores)]) / np.abs(score[:len(scores)])):.3e}, edges {edges}")
    assert status == 0 and (na, nn) == (ona, onn) and len(top) == 11
    assert list(codes) == top
    np.testing.assert_allclose(scores, score, rtol=1e-10, atol=0)
    assert edges == k * edges_per_iteration(name)
    assert info["iters"] == k


# ---------------------------------------------------------------------------- 1: the count is honoured
@pytest.mark.parametrize("name", ["A", "B"])
def test_count_honoured_against_oracle(ctx, wins, name):
    top25, sc25, _, _ = oracle_rank(name, 25)
    top60, sc60, _, _ = oracle_rank(name, 60)
    moved = float(np.max(np.abs(sc60 - sc25) / np.abs(sc25)))
    print(f"oracle {name}: 60 vs 25 iterations move the scores by {moved:.3e} relative")
    assert top25 == top60 and moved > 1e-7, "the window no longer tells 60 iterations from 25"
    check_against_oracle(name, rank(ctx, [wins[name]], iters=60)[0], 60, "rank_windows")
    check_against_oracle(name, single(ctx, wins[name], iters=60), 60, "rca_window")
    top40, sc40, _, _ = oracle_rank(name, 40)
    for what, ((c32, s32, na, nn, edges, status), info) in (
            ("rank_windows", rank(ctx, [wins[name]], iters=40, precision="fp32")[0]),
            ("rca_window", single(ctx, wins[name], iters=40, precision="fp32"))):
        assert status == 0 and info["iters"] == 40 and edges == 40 * edges_per_iteration(name)
        assert list(c32[:5]) == top40[:5], what
        np.testing.assert_allclose(s32, sc40, rtol=1e-4, atol=0)


# ---------------------------------------------------------------------------- 2: the report
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("iters", [1, 2, 25, 60])
def test_report_against_oracle(ctx, wins, name, iters):
    want = oracle_resid(name, iters)
    for what, (res, info) in (("rank_windows", rank(ctx, [wins[name]], iters=iters)[0]),
                              ("rca_window", single(ctx, wins[name], iters=iters))):
        got = (info["resid_normal"], info["resid_anomaly"])
        print(f"{what} {name} iters={iters}: residuals {got}, oracle {want}")
        assert info["iters"] == iters
        assert abs(got[0] - want[0]) <= ATOL64 and abs(got[1] - want[1]) <= ATOL64
    (res, info), = rank(ctx, [wins[name]], iters=iters, precision="fp32")
    got = (info["resid_normal"], info["resid_anomaly"])
    print(f"fp32 {name} iters={iters}: residuals {got}")
    assert info["iters"] == iters
    for g, w in zip(got, want):
        assert np.isfinite(g) and g >= 0.0 and abs(g - w) <= ATOL32


def test_report_of_a_graph_past_one_residual_block(ctx, wins):
    """Up to 4096 ops (RESID_OPS) a graph's one k_resid block stores the report's word; past it the
    graph's blocks meet in an integer max over zeroed words.  Window D's graph of normal traces takes
    the second form; the tol form beside it (never reached: it runs to iters) reads the same value
    out of its history."""
    sizes = [g.N for g, _ in oracle_graphs("D")[2]]
    print("window D: ops per graph", sizes)
    assert sizes[0] <= 4096 < sizes[1]
    want = oracle_resid("D", 3)
    fixed = rank(ctx, [wins["D"]], iters=3)[0]
    for what, (res, info) in (("rank_windows", fixed), ("rca_window", single(ctx, wins["D"], iters=3))):
        got = (info["resid_normal"], info["resid_anomaly"])
        print(f"{what} D iters=3: residuals {got}, oracle {want}")
        assert res[5] == 0 and info["iters"] == 3 and res[4] == 3 * edges_per_iteration("D")
        assert abs(got[0] - want[0]) <= ATOL64 and abs(got[1] - want[1]) <= ATOL64
    assert_same(rank(ctx, [wins["D"]], iters=3, tol=1e-300, check_every=2)[0], fixed, "history against report")
    assert_same(rank(ctx, [wins["A"], wins["D"]], iters=3)[1], fixed, "beside one-block graphs")


# ---------------------------------------------------------------------------- 3: the default is the old call
def test_default_is_the_old_call_bitwise(ctx, wins):
    import bench
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows

    ws = [wins["A"], wins["B"], wins["C"], (wins["A"][0], 0, 1) + wins["A"][3:]]   # the last: no trace in [0, 1] ns
    plain = rank_windows(ctx, ws)
    counted = rank_windows(ctx, ws, iters=25)
    info = []
    reported = rank_windows(ctx, ws, iters=25, info=info)
    for got in (counted, reported):
        for a, b in zip(plain, got):
            assert list(a[0]) == list(b[0]) and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]
    for w, r, rep in zip(ws[:3], plain[:3], info[:3]):
        e, c1, s1, na1, nn1 = bench.run_window(ctx, w[0], w[1], w[2], w[3], w[4], _lib.MR_FP64)   # mr_rca_window
        assert r[5] == 0 and len(r[0]) == 11
        assert list(r[0]) == list(c1) and r[1].tobytes() == s1.tobytes() and r[2:5] == (na1, nn1, e)
        assert rep["iters"] == 25 and rep["resid_normal"] > 0.0 and rep["resid_anomaly"] > 0.0
    assert plain[3][5] == _lib.MR_ERR_VALUE and len(plain[3][0]) == 0 and plain[3][4] == 0
    assert info[3] == {"iters": 0, "resid_normal": 0.0, "resid_anomaly": 0.0}


# ---------------------------------------------------------------------------- 4: forms and groupings
def test_forms_and_groupings_agree_bitwise(ctx, wins, wins_general, monkeypatch):
    """A, B, C at iters=40 under every form and grouping, results and reports bit for bit: one call /
    a window per call / rca_window, one-window groups and chunks, k_fx_b every iteration (MR_TR_PF=0),
    the spectrum after the words (MR_WIN_SPEC_EARLY=0) -- all against the default call; and the
    general window build (tables uploaded under MR_NO_LO=1, MR_NO_LO_WIN=1, mr_rca_window's general
    path) under the same forms, all against one another.  Between the two builds a trace's entries
    are summed in another order: there the project's 1e-12 holds, as it does for the plain entries
    (tests/test_gpu_rca.py::test_windows_batch_layout_order_equals_general_build)."""
    names = ["A", "B", "C"]
    base = rank(ctx, [wins[n] for n in names], iters=40)
    for (res, info), n in zip(base, names):
        assert res[5] == 0 and len(res[0]) == 11 and info["iters"] == 40
        assert res[4] == 40 * edges_per_iteration(n)

    def under(env, fn):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = fn()
        for k in env:
            monkeypatch.delenv(k)
        return out

    batch = lambda w: rank(ctx, [w[n] for n in names], iters=40)   # noqa: E731
    alone = lambda w: [rank(ctx, [w[n]], iters=40)[0] for n in names]   # noqa: E731
    one = lambda w: [single(ctx, w[n], iters=40) for n in names]   # noqa: E731
    layout = {
        "a window per call": under({}, lambda: alone(wins)),
        "rca_window": under({}, lambda: one(wins)),
        "group 1, chunk 1": under({"MR_WIN_GROUP": "1", "MR_WIN_CHUNK": "1"}, lambda: batch(wins)),
        "k_fx_b every iteration": under({"MR_TR_PF": "0"}, lambda: batch(wins)),
        "k_fx_b every iteration, a window per call": under({"MR_TR_PF": "0"}, lambda: alone(wins)),
        "spectrum after the words, a window per call": under({"MR_WIN_SPEC_EARLY": "0"}, lambda: alone(wins)),
    }
    general = {
        "tables without a layout order": under({}, lambda: batch(wins_general)),
        "tables without a layout order, a window per call": under({}, lambda: alone(wins_general)),
        "tables without a layout order, group 1, chunk 1":
            under({"MR_WIN_GROUP": "1", "MR_WIN_CHUNK": "1"}, lambda: batch(wins_general)),
        "tables without a layout order, k_fx_b every iteration": under({"MR_TR_PF": "0"}, lambda: batch(wins_general)),
        "tables without a layout order, rca_window (its general path)": under({}, lambda: one(wins_general)),
        "MR_NO_LO_WIN": under({"MR_NO_LO_WIN": "1"}, lambda: batch(wins)),
        "MR_NO_LO_WIN, rca_window (its general path)": under({"MR_NO_LO_WIN": "1"}, lambda: one(wins)),
    }
    bad = []
    for family, ref in ((layout, base), (general, general["tables without a layout order"])):
        for what, got in family.items():
            for n, a, b in zip(names, ref, got):
                try:
                    assert_same(a, b, f"{what}: window {n}")
                except AssertionError as e:
                    bad.append(str(e).splitlines()[0])
    print("\n".join(bad))
    assert not bad
    # the two builds sum a trace's entries in another order (tests/test_gpu_rca.py::
    # test_windows_batch_layout_order_equals_general_build): the same lists and counts, scores to 1e-12
    for n, (ra, ia), (rb, ib) in zip(names, base, general["tables without a layout order"]):
        assert list(ra[0]) == list(rb[0]) and ra[2:] == rb[2:] and ia["iters"] == ib["iters"], n
        np.testing.assert_allclose(ra[1], rb[1], rtol=1e-12, atol=0)
        for k in ("resid_normal", "resid_anomaly"):
            assert abs(ia[k] - ib[k]) <= ATOL64, (n, k)


# ---------------------------------------------------------------------------- 5: a collision rerun keeps the count
def test_collision_rerun_keeps_the_count(ctx, wins_general, monkeypatch, capfd):
    """MR_KIND_TEST_COLLIDE makes the first attempt's kind hashing collide (general-build tables): the
    group reruns synchronously -- further attempts, counted by MR_PR_HOST_TIMING's line per attempt --
    with the call's 40 iterations, not the reference's 25, and its report replaces the first one."""
    monkeypatch.setenv("MR_PR_HOST_TIMING", "1")

    def attempts(fn):
        capfd.readouterr()
        out = fn()
        return out, capfd.readouterr().err.count("[pagerank host")

    names = ["A", "B", "C"]
    for ws in ([wins_general["A"]], [wins_general[n] for n in names]):
        base, n_base = attempts(lambda: rank(ctx, ws, iters=40))
        at25 = rank(ctx, ws, iters=25)
        assert all(a[0][1].tobytes() != b[0][1].tobytes() for a, b in zip(base, at25)), \
            "25 and 40 iterations rank alike: the case no longer tells a rerun with 25 apart"
        monkeypatch.setenv("MR_KIND_TEST_COLLIDE", "1")
        coll, n_coll = attempts(lambda: rank(ctx, ws, iters=40))
        monkeypatch.delenv("MR_KIND_TEST_COLLIDE")
        # (the group's enqueued attempt, then the rerun's first seed -- the knob collides it again -- and its second)
        assert (n_base, n_coll) == (1, 3), "the collision did not rerun the group"
        for a, b in zip(base, coll):
            assert a[0][5] == 0 and a[1]["iters"] == 40
            assert_same(a, b, "collision rerun")
    base, n_base = attempts(lambda: single(ctx, wins_general["A"], iters=40))
    monkeypatch.setenv("MR_KIND_TEST_COLLIDE", "1")   # (mr_rca_window's general path: the synchronous form's retry loop)
    coll, n_coll = attempts(lambda: single(ctx, wins_general["A"], iters=40))
    assert (n_base, n_coll) == (1, 2), "the collision did not retry"
    assert_same(base, coll, "collision retry of the synchronous form")


# ---------------------------------------------------------------------------- 6: stop at a tolerance
EVERY, MAX_ITERS = 5, 200


def oracle_stop(names, tol):
    """The first check at which every graph of the windows is <= tol, with the margins the case needs:
    a factor 1.5 between tol and the largest residual at the stop and at the check before."""
    worst = lambda k: max(max(oracle_resid(n, k)) for n in names)   # noqa: E731
    stop = next(k for k in range(EVERY, 100, EVERY) if worst(k) <= tol)
    print(f"oracle {names} tol {tol}: stop at {stop}, largest residual there {worst(stop):.3e}, "
          f"at the check before {worst(stop - EVERY):.3e}")
    assert stop > EVERY
    assert worst(stop) * 1.5 <= tol and worst(stop - EVERY) >= 1.5 * tol, "a check sits too close to tol to pin the stop"
    return stop


@pytest.mark.parametrize("names,tol,expect", [(("A",), 2e-9, 60), (("B",), 1e-9, 70), (("A", "B", "C"), 1e-9, 70)],
                         ids=["A", "B", "ABC"])
def test_stop_at_a_tolerance(ctx, wins, names, tol, expect):
    stop = oracle_stop(names, tol)
    assert stop == expect, "the generator drifted: the issue's table no longer holds"
    ws = [wins[n] for n in names]
    got = rank(ctx, ws, iters=MAX_ITERS, tol=tol, check_every=EVERY)
    fixed = rank(ctx, ws, iters=stop)
    for n, (res, info), f in zip(names, got, fixed):
        want = oracle_resid(n, stop)
        print(f"{n}: iters {info['iters']}, residuals {info['resid_normal']:.3e} {info['resid_anomaly']:.3e}, "
              f"oracle {want[0]:.3e} {want[1]:.3e}")
        assert res[5] == 0 and info["iters"] == stop
        assert res[4] == stop * edges_per_iteration(n)
        for g, w in zip((info["resid_normal"], info["resid_anomaly"]), want):
            assert g <= tol and abs(g - w) <= ATOL64
        assert_same((res, info), f, f"tol form against iters={stop}: window {n}")
    if len(names) == 1:   # mr_rca_window_ex takes the same route
        assert_same(single(ctx, ws[0], iters=MAX_ITERS, tol=tol, check_every=EVERY), fixed[0], "rca_window, tol form")


def test_fp32_tolerance_below_its_floor_runs_to_iters(ctx, wins):
    (res, info), = rank(ctx, [wins["A"]], iters=40, tol=1e-9, check_every=EVERY, precision="fp32")
    print("fp32, tol 1e-9:", info)
    assert res[5] == 0 and info["iters"] == 40
    assert_same((res, info), rank(ctx, [wins["A"]], iters=40, precision="fp32")[0], "fp32 tol form against iters=40")


def test_library_rejects_bad_counts(ctx, wins):
    """MR_ERR_ARG from the C entries themselves (the Python keywords are checked before them)."""
    import ctypes as C

    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    dev, t0, t1, a3, ok = wins["A"]
    a3, ok = np.array(a3), np.array(ok)
    lib = _lib.load()
    for iters, tol, every in ((0, 0.0, 1), (25, 0.0, 0), (25, -1.0, 5), (25, float("nan"), 5)):
        codes, scores = np.zeros(11, np.int32), np.zeros(11)
        n_out, na, nn, edges, st = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        rc = lib.mr_rca_window_ex(ctx.h, dev.h, t0, t1, ptr(a3, C.c_double), ptr(ok, C.c_uint8), 0, 5, _lib.MR_FP64,
                                  ptr(codes, C.c_int32), ptr(scores, C.c_double), C.byref(n_out), C.byref(edges),
                                  C.byref(na), C.byref(nn), iters, tol, every, None, None)
        assert rc == _lib.MR_ERR_ARG, (iters, tol, every)
        spans = (_lib.P * 1)(dev.h)
        t0a, t1a = np.array([t0], np.int64), np.array([t1], np.int64)
        a3p, okp = (C.c_void_p * 1)(a3.ctypes.data), (C.c_void_p * 1)(ok.ctypes.data)
        rc = lib.mr_windows_batch_ex(ctx.h, 1, spans, ptr(t0a, C.c_int64), ptr(t1a, C.c_int64), a3p, okp, 0, 5,
                                     _lib.MR_FP64, ptr(codes, C.c_int32), ptr(scores, C.c_double), C.byref(n_out),
                                     C.byref(edges), C.byref(na), C.byref(nn), C.byref(st), iters, tol, every, None, None)
        assert rc == _lib.MR_ERR_ARG, (iters, tol, every)


# ---------------------------------------------------------------------------- 7: the driver
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
    return buf.getvalue().splitlines(), err


def test_driver_passes_the_count_on(tmp_path, monkeypatch):
    from microrank_amd import synth

    case = load_golden("stream.json")
    _, adf = synth.stream_dataframes(**case["params"])
    monkeypatch.chdir(tmp_path)
    default, err = _driver(adf, case)
    assert err == case.get("driver_error")
    assert _driver(adf, case, iters=25) == (default, err)
    csv25 = open("result.csv").read() if os.path.exists("result.csv") else None
    more, err60 = _driver(adf, case, iters=60)
    assert err60 == err and len(more) == len(default)
    counts = ("anormaly_trace", "total_trace", "anomaly_list", "normal_list", "total")
    scored = lambda ln: ln.startswith("[") or ": " in ln   # noqa: E731
    assert [ln for ln in more if ln.startswith(counts)] == [ln for ln in default if ln.startswith(counts)]
    assert [scored(ln) for ln in more] == [scored(ln) for ln in default]
    assert any(ln.startswith("[") for ln in default)
    assert more != default, "60 iterations print the scores of 25"
    if csv25 is not None:
        assert open("result.csv").read() != csv25
