"""Wide graphs (N > 16384: hot ops through k_tr_a's LDS walk, the cold tail through k_cold_trace /
k_cold_ops) in batches, in launches mixed with narrow and tile-path graphs, kind-compressed, under
mr_pagerank_converge and through the window entries -- every other test of the wide path ranks one
graph with one plain call.  Cases, their shape facts and their oracle results: tests/wide_cases.py
(the shapes are asserted on the CPU by tests/test_wide_cases.py).

Reference: the numpy oracle -- weights 1e-10 (fp64) / 1e-4 (fp32) relative on EVERY op of a wide
graph, zero-coverage ops included (the narrow fp32 cases N1 / N2 through _assert_fp32's mask, as the
existing mixed-batch test does); kinds, preference and coverage byte-equal to the graph ranked alone
and equal to the oracle's; reruns bitwise.

Batched against alone, max relative difference of a graph's weights (measured on an MI355X, printed
by every test; the table is in DESIGN.md, "Wide graphs in batches"):
  * fp64: byte-equal in every batch below, wide and narrow graphs alike -- the cold rows' fixed-point
    scale comes from the graph's own cold_span and the partial rows' from its own tiles, so the
    expected benign cause of a difference does not arise.  Asserted at the project's bound for
    narrow graphs, 1e-12 (test_gpu_setup_paths).
  * fp32, [W1, W2] and [W2, W1, W1'] (alone and batched on the float-su variant, EXT 10): measured
    0, so 4x the measured difference is byte-equality, which is asserted.
  * fp32, mixed launches: the wide graph changes kernel variant (EXT 10 alone; EXT 2 with su rounded
    to float beside a narrow graph; the general walk when the launch leaves su-in-LDS), so only the
    oracle bound is asserted and the difference printed: W1 1.1e-7 beside N1 or N2, W2 3.5e-8 in
    [N2, W2, TP, N1], byte-equal beside TP.

What the tests caught: on the parent of the commit that added them, W1 beside N2 was off by up to
40 % (k_cold_trace left most tiles' cold sums unwritten when the launch left su-in-LDS; fixed with
Launch::cold_all) -- test_mixed_batches[W1-N2-*], [N2-W2-TP-N1-*], the WS-mixed window tests and
test_windows_batch_with_wide_graphs failed there.
"""
import ctypes as C

import numpy as np
import pytest

import wide_cases as wc
from test_gpu_general_graphs import RTOL64, _assert_fp32, _assert_fp64
from test_gpu_pagerank_converge import ATOL32, ATOL64

pytestmark = pytest.mark.gpu

# a graph's weights batched against ranked alone (module docstring): fp64 the project's bound (measured
# byte-equal); fp32 among wide graphs only 4x the measured 0
BATCH_VS_ALONE_64 = 1e-12
BATCH_VS_ALONE_32_WIDE = 0.0

ANOMALY = {"W1": False, "W2": True, "W1'": True, "N1": True, "N2": False, "TP": True}
FP32_MASKED = ("N1", "N2")   # narrow graphs: ops reached only through the alpha chain (test_c4's rule)


def _base(name):
    return name.rstrip("'")


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


@pytest.fixture(scope="module")
def dev(ctx):
    """name -> DeviceGraph, uploaded once ("W1'": a second upload of W1)."""
    from microrank_amd.graph import DeviceGraph

    up = {}

    def get(name):
        if name not in up:
            up[name] = DeviceGraph.upload(ctx, wc.case(_base(name)).hg)
        return up[name]

    yield get
    for dg in up.values():
        dg.close()


@pytest.fixture(scope="module")
def alone(dev):
    """(name, precision) -> (weights, coverage, kinds, preference) of the graph ranked by one plain
    call with its flag of ANOMALY, computed at first use and kept: later tests compare with bytes an
    earlier state of the handle gave."""
    got = {}

    def get(name, precision):
        if (name, precision) not in got:
            dg = dev(name)
            dg.pagerank(ANOMALY[name], precision=precision)
            got[(name, precision)] = dg.fetch(kinds=True)
        return got[(name, precision)]

    return get


def _batch(ctx, dgs, anomaly, precision, iters=25):
    from microrank_amd import _lib

    hs = (_lib.P * len(dgs))(*[dg.h for dg in dgs])
    an = (C.c_int * len(dgs))(*[int(a) for a in anomaly])
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    return _lib.load().mr_pagerank_batch(ctx.h, hs, an, len(dgs), 0.85, 0.01, iters, prec, 0)


def _rel(w, w_a):
    m = w_a != 0
    return float(np.max(np.abs(w - w_a)[m] / np.abs(w_a[m]))) if m.any() else 0.0


def _against_oracle(name, w, cov, kind, anomaly, precision, what):
    c = wc.case(_base(name))
    v, w_ref, cov_ref = c.ref[anomaly]
    np.testing.assert_array_equal(kind, c.kind, err_msg=what)
    np.testing.assert_array_equal(cov, cov_ref, err_msg=what)
    assert np.isfinite(w).all(), what
    if precision == "fp64":
        _assert_fp64(w, w_ref, what)
    else:
        _assert_fp32(w, w_ref, _base(name) in FP32_MASKED, what)


def _run_batch(ctx, dev, alone, names, precision, bound_alone):
    """One mr_pagerank_batch over `names`, twice: every graph against itself ranked alone and against
    the oracle; the second call's weights bitwise the first's.  Returns the largest difference from
    alone over the wide graphs."""
    ref = [alone(n, precision) for n in names]
    dgs = [dev(n) for n in names]
    an = [ANOMALY[n] for n in names]
    ctx.check(_batch(ctx, dgs, an, precision), "mr_pagerank_batch")
    first, worst = [], 0.0
    for n, dg, (w_a, cov_a, k_a, p_a) in zip(names, dgs, ref):
        w, cov, k, p = dg.fetch(kinds=True)
        what = f"batch {names} {precision}: {n}"
        assert (k.tobytes(), p.tobytes(), cov.tobytes()) == (k_a.tobytes(), p_a.tobytes(), cov_a.tobytes()), what
        diff = _rel(w, w_a)
        print(f"{what}: batched vs alone byte-equal {w.tobytes() == w_a.tobytes()}, max rel diff {diff:.3e}")
        _against_oracle(n, w, cov, k, ANOMALY[n], precision, what)
        if bound_alone is not None:
            np.testing.assert_allclose(w, w_a, rtol=bound_alone, atol=0, err_msg=what)
        if wc.case(_base(n)).shape.wide:
            worst = max(worst, diff)
        first.append(w)
    ctx.check(_batch(ctx, dgs, an, precision), "mr_pagerank_batch")
    for n, dg, w in zip(names, dgs, first):
        assert dg.fetch()[0].tobytes() == w.tobytes(), f"batch {names} {precision}: {n} rerun not bitwise"
    return worst


# ---------------------------------------------------------------------------- 1: wide graphs together
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("names", [("W1", "W2"), ("W2", "W1", "W1'")], ids="-".join)
def test_batch_of_wide_graphs(ctx, dev, alone, names, precision):
    """Two wide graphs (split_fa / split_fb, each its own k_cold_ops between the side-stream events,
    cold_rw / cx_scale / NA per graph; fp32: EXT 10 as alone) and three (the block -> graph search),
    the third a second upload of W1 with the other anomaly flag.  Measured batched vs alone:
    byte-equal in both precisions; asserted at 1e-12 (fp64) and at byte-equality (fp32: 4x the
    measured 0)."""
    bound = BATCH_VS_ALONE_64 if precision == "fp64" else BATCH_VS_ALONE_32_WIDE
    worst = _run_batch(ctx, dev, alone, list(names), precision, bound)
    print(f"wide batch {names} {precision}: largest batched-vs-alone difference {worst:.3e}")


# ---------------------------------------------------------------------------- 2: mixed launches
MIXES = [("W1", "N1"), ("W1", "N2"), ("W2", "TP"), ("N2", "W2", "TP", "N1")]


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("names", MIXES, ids="-".join)
def test_mixed_batches(ctx, dev, alone, names, precision, reverse):
    """A wide graph beside a narrow fused one with su in LDS (N1: fp32 walks the wide graph's
    float-rounded su on the EXT 2 kernel), beside one whose su is out of LDS (N2: the launch leaves
    WV_SU_ALL, no kernel of that mode has a short-tile walk, so k_cold_trace sums every tile of the
    wide graph), beside a tile-path graph (k_iter_a / k_iter_b in the same iteration), and all four
    kinds together (N1 is not relabelled: WV_SU_GLOBAL).  fp64: each graph within BATCH_VS_ALONE_64
    of itself alone; fp32: the oracle bound only (the variant changes), the difference printed.
    After the batch N1 ranked alone gives its earlier bytes: no ring state leaks."""
    names = list(reversed(names)) if reverse else list(names)
    n1_before = alone("N1", precision)[0]
    worst = _run_batch(ctx, dev, alone, names, precision, BATCH_VS_ALONE_64 if precision == "fp64" else None)
    print(f"mixed batch {names} {precision}: largest batched-vs-alone difference of a wide graph {worst:.3e}")
    dg = dev("N1")
    dg.pagerank(ANOMALY["N1"], precision=precision)
    assert dg.fetch()[0].tobytes() == n1_before.tobytes(), "N1 alone after the batch: not its earlier bytes"


# ---------------------------------------------------------------------------- 3: kind compression
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_kind_compressed_wide_graph(ctx, precision, monkeypatch):
    """WK (W1 with its traces repeated: 6000 kinds of 12000 traces): the representatives' graph is wide
    too and carries multiplicities and cold sums (EXT 3; fp32: su32 without the float-su variant).
    Compressed vs uncompressed 1e-10 (fp64, test_kind_compressed_c2_matches_uncompressed's bound) and
    vs the oracle; a second call through the cached representatives' graph: the same bytes; the
    other anomaly flag through the cache: the oracle's, and bitwise a call that rebuilds the graph."""
    from microrank_amd.graph import DeviceGraph

    c = wc.case("WK")
    dg = DeviceGraph.upload(ctx, c.hg)
    dg.pagerank(True, precision=precision)
    w0, cov0, k0, _ = dg.fetch(kinds=True)
    _against_oracle("WK", w0, cov0, k0, True, precision, f"WK uncompressed {precision}")
    dg.pagerank(True, precision=precision, compress_kinds=True)
    w1, cov1, k1, _ = dg.fetch(kinds=True)
    print(f"WK {precision}: compressed vs uncompressed max rel diff {_rel(w1, w0):.3e}")
    np.testing.assert_array_equal(cov1, cov0)
    np.testing.assert_array_equal(k1, k0)
    _against_oracle("WK", w1, cov1, k1, True, precision, f"WK compressed {precision}")
    if precision == "fp64":
        np.testing.assert_allclose(w1, w0, rtol=1e-10, atol=0)
    dg.pagerank(True, precision=precision, compress_kinds=True)
    assert dg.fetch()[0].tobytes() == w1.tobytes(), "second compressed call: not the first one's bytes"
    dg.pagerank(False, precision=precision, compress_kinds=True)
    w2, cov2, k2, _ = dg.fetch(kinds=True)
    _against_oracle("WK", w2, cov2, k2, False, precision, f"WK compressed, flag flipped {precision}")
    assert w2.tobytes() != w1.tobytes()
    monkeypatch.setenv("MR_KC_NOCACHE", "1")
    dg.pagerank(False, precision=precision, compress_kinds=True)
    monkeypatch.delenv("MR_KC_NOCACHE")
    assert dg.fetch()[0].tobytes() == w2.tobytes(), "cached representatives' graph: not a rebuild's bytes"
    dg.close()


# ---------------------------------------------------------------------------- 4: the converge contract
def _converge_handles(dev):
    names = [n for n, _ in wc.CONVERGE_BATCH]
    return names, [dev(n) for n in names], [a for _, a in wc.CONVERGE_BATCH]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_converge_fixed_count_over_wide_and_narrow(ctx, dev, precision):
    """mr_pagerank_converge(tol = 0, max_iters = 7) over [W1, N1, W2]: weights and coverage bytewise
    those of mr_pagerank_batch(iters = 7) on the same handles; the residual history against the
    oracle's max-normalised iterates (2e-10 fp64 / 2e-4 fp32 absolute, test_gpu_pagerank_converge)."""
    from microrank_amd.graph import converge_batch

    K = wc.CONVERGE_FIXED
    names, dgs, an = _converge_handles(dev)
    reps = converge_batch(ctx, dgs, an, tol=0.0, max_iters=K, precision=precision)
    got = [dg.fetch() for dg in dgs]
    ctx.check(_batch(ctx, dgs, an, precision, iters=K), "mr_pagerank_batch")
    atol = ATOL64 if precision == "fp64" else ATOL32
    for n, a, dg, rep, (w, cov) in zip(names, an, dgs, reps, got):
        want = wc.history(n, a, K, precision)
        err = np.abs(rep["residuals"] - want)
        print(f"converge {n} {precision}: max |gpu - oracle| residual {err.max():.3e} at k={int(err.argmax()) + 1}, "
              f"oracle last {want[-1]:.3e}")
        assert rep["iters"] == K and rep["residuals"].shape == (K,) and rep["converged_at"] is None
        assert (err <= atol).all(), (n, rep["residuals"], want)
        w_b, cov_b = dg.fetch()
        assert np.isfinite(w_b).all() and (w_b != 0).any()
        assert w.tobytes() == w_b.tobytes(), f"{n}: converge(tol=0, 7) weights are not batch(iters=7)'s bytes"
        assert cov.tobytes() == cov_b.tobytes()
        if precision == "fp64":
            np.testing.assert_allclose(w, wc.weights_after(n, a, K), rtol=RTOL64, atol=0)


def test_converge_stops_at_a_check_over_wide_and_narrow(ctx, dev):
    """A tolerance W1 reaches at its 4th iteration (the oracle's history, margins asserted by
    wide_cases.converge_stop): with a check every 3 iterations the batch stops at K = 6 < max_iters,
    each graph's converged_at is the oracle's, and the weights are bytewise batch(iters = K)'s."""
    from microrank_amd.graph import converge_batch

    K, first = wc.converge_stop()
    names, dgs, an = _converge_handles(dev)
    reps = converge_batch(ctx, dgs, an, tol=wc.CONVERGE_TOL, check_every=wc.CONVERGE_EVERY, max_iters=wc.CONVERGE_MAX)
    got = [dg.fetch() for dg in dgs]
    ctx.check(_batch(ctx, dgs, an, "fp64", iters=K), "mr_pagerank_batch")
    for n, a, dg, rep, f, (w, cov) in zip(names, an, dgs, reps, first, got):
        want = wc.history(n, a, wc.CONVERGE_MAX)[:K]
        print(f"converge to {wc.CONVERGE_TOL:g} {n}: stopped at {rep['iters']}, converged_at {rep['converged_at']}, "
              f"residuals {rep['residuals']}")
        assert rep["iters"] == K and rep["converged_at"] == f
        assert (np.abs(rep["residuals"] - want) <= ATOL64).all()
        w_b, cov_b = dg.fetch()
        assert w.tobytes() == w_b.tobytes(), f"{n}: weights after the stop are not batch(iters={K})'s bytes"
        assert cov.tobytes() == cov_b.tobytes()
        np.testing.assert_allclose(w, wc.weights_after(n, a, K), rtol=RTOL64, atol=0)


# ---------------------------------------------------------------------------- 5: the window entries
@pytest.fixture(scope="module")
def ws_dev(ctx):
    from microrank_amd.preprocess_data import DeviceSpans

    d = DeviceSpans(ctx, wc.ws_table())
    yield d
    d.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("name", wc.WINDOWS)
def test_rca_window_with_wide_graphs(ctx, ws_dev, name, precision):
    """mr_rca_window over more than 16384 pod-ops: the window's pair of graphs arrives at the batch
    as two wide graphs (WS) or as a narrow one with su out of LDS beside a wide one (WS-mixed); the
    spectrum sorts > 23k nodes.  Counts and top list the oracle's, scores 1e-10 (fp64); fp32 the
    top-5 and 1e-4 (test_c3_window_against_oracle)."""
    import bench
    from microrank_amd import _lib

    _, t0, t1, a3, ok = wc.window(name)
    top, score, na, nn, _ = wc.window_expected(name)
    assert len(top) == 11
    prec = _lib.MR_FP64 if precision == "fp64" else _lib.MR_FP32
    e, codes, scores, gna, gnn = bench.run_window(ctx, ws_dev, t0, t1, np.array(a3), np.array(ok), prec)
    print(f"{name} {precision}: max rel score diff {_rel(scores, score[:len(scores)]):.3e}, edges {e}")
    assert (gna, gnn) == (na, nn)
    if precision == "fp64":
        assert list(codes) == top
        np.testing.assert_allclose(scores, score, rtol=1e-10, atol=0)
    else:
        assert list(codes[:5]) == top[:5]
        np.testing.assert_allclose(scores, score, rtol=1e-4, atol=0)


def test_windows_batch_with_wide_graphs(ctx, ws_dev):
    """rank_windows over [WS, WS-mixed, WS, an empty window]: each non-empty window equals its
    standalone mr_rca_window (top list, counts, edges; scores 1e-12 as in
    test_windows_batch_matches_standalone), the repeated window is bytewise itself, the empty one is
    flagged MR_ERR_VALUE."""
    import bench
    from microrank_amd import _lib
    from microrank_amd.online_rca import rank_windows

    wins = []
    for name in ("WS", "WS-mixed", "WS"):
        _, t0, t1, a3, ok = wc.window(name)
        wins.append((ws_dev, t0, t1, np.array(a3), np.array(ok)))
    wins.append((ws_dev, 0, 1, wins[0][3], wins[0][4]))   # no trace in [0, 1] ns
    got = rank_windows(ctx, wins)
    for name, w, (codes, scores, na, nn, edges, status) in zip(("WS", "WS-mixed", "WS"), wins[:3], got[:3]):
        assert status == 0
        e, c1, s1, na1, nn1 = bench.run_window(ctx, w[0], w[1], w[2], w[3], w[4], _lib.MR_FP64)
        print(f"windows batch {name}: vs standalone byte-equal {scores.tobytes() == s1.tobytes()}, "
              f"max rel diff {_rel(scores, s1):.3e}")
        assert (na, nn, edges) == (na1, nn1, e)
        assert list(codes) == list(c1)
        np.testing.assert_allclose(scores, s1, rtol=1e-12, atol=0)
        top, score, ona, onn, _ = wc.window_expected(name)
        assert (na, nn) == (ona, onn) and list(codes) == top
        np.testing.assert_allclose(scores, score, rtol=1e-10, atol=0)
    assert got[0][0].tolist() == got[2][0].tolist() and got[0][1].tobytes() == got[2][1].tobytes()
    assert got[3][5] == _lib.MR_ERR_VALUE


def test_rca_window_iteration_count_and_residuals_on_wide_graphs(ctx, ws_dev):
    """mr_rca_window_ex(iters = 7) with a report on WS: the top list and scores of a fixed-count call
    without one, the oracle's 7-iteration window (1e-10), and both residuals finite, > 0 and the
    oracle's (2e-10 absolute)."""
    import types

    from microrank_amd.online_rca import rca_window
    from test_gpu_window_iters import single

    _, t0, t1, a3, ok = wc.window("WS")
    w = (ws_dev, t0, t1, np.array(a3), np.array(ok))
    tab = types.SimpleNamespace(n_svcops=len(a3), svcop_names=list(range(len(a3))), podop_names=None)
    slo_d = {i: [float(a3[i]), 0.0] for i in range(len(a3))}
    plain = rca_window(None, t0, t1, slo_d, ctx=ctx, table=tab, dev=ws_dev, iters=7)
    (codes, scores, na, nn, edges, _), info = single(ctx, w, iters=7)
    print(f"WS iters=7: report {info}")
    assert info["iters"] == 7
    assert list(codes) == plain["top"] and scores.tolist() == plain["score"]
    r = (info["resid_normal"], info["resid_anomaly"])
    assert all(np.isfinite(x) and x > 0 for x in r)
    top, score, ona, onn, resid = wc.window_expected("WS", 7)
    assert (na, nn) == (ona, onn) and list(codes) == top
    np.testing.assert_allclose(scores, score, rtol=1e-10, atol=0)
    assert abs(r[0] - resid[0]) <= ATOL64 and abs(r[1] - resid[1]) <= ATOL64, (r, resid)


# ---------------------------------------------------------------------------- 6: refusals stay refusals
def test_hot_layout_of_eight_ops_beside_a_wide_graph_is_refused(ctx, monkeypatch):
    """A narrow graph laid out with 8 register-accumulated hot ops (forced: MR_TR_HOT_MIN=0,
    MR_TR_HOT_FRAC=0, MR_TR_HOT=8) cannot share a launch with a wide graph, whose kernel variant
    carries HOT_MAX_WIDE = 4 accumulators: MR_ERR_ARG, and the context ranks W1 alone afterwards."""
    from microrank_amd import _lib, synth
    from microrank_amd.graph import DeviceGraph

    for k, v in (("MR_TR_HOT_MIN", "0"), ("MR_TR_HOT_FRAC", "0"), ("MR_TR_HOT", "8")):
        monkeypatch.setenv(k, v)
    hot = synth.big_graph(1000, 3000, seed=21)
    cov = np.bincount(hot.sr_ops, minlength=hot.N)
    assert int((cov * 8 >= hot.T).sum()) >= 8, "fewer than 8 ops in an eighth of the traces: no 8-op layout"
    dg_hot = DeviceGraph.upload(ctx, hot)
    dg_w1 = DeviceGraph.upload(ctx, wc.case("W1").hg)
    dg_hot.pagerank(True)   # alone it ranks (and is prepared with its hot-op layout)
    rc = _batch(ctx, [dg_hot, dg_w1], [True, False], "fp64")
    msg = (_lib.load().mr_last_error(ctx.h) or b"").decode(errors="replace")
    print("refusal:", rc, msg)
    assert rc == _lib.MR_ERR_ARG and "beside a wide graph" in msg
    rc = _batch(ctx, [dg_w1, dg_hot], [False, True], "fp64")
    assert rc == _lib.MR_ERR_ARG
    dg_w1.pagerank(False)
    w, cov_w, k, _ = dg_w1.fetch(kinds=True)
    _against_oracle("W1", w, cov_w, k, False, "fp64", "W1 alone after the refusal")
    dg_hot.close()
    dg_w1.close()
