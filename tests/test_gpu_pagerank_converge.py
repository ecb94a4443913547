"""mr_pagerank_converge on the GPU: the residual history against the oracle's, the early stop, and
the contract that a call which ran K iterations leaves the weights of a plain K-iteration ranking,
bit for bit.

The expected history comes from the unchanged oracle: s_k = orc.power_iteration(g, v, iters=k) for
k = 1..K (the max-normalised vector the reference holds after k iterations), s_0 = ones(N)/(N+T),
resid[k-1] = max|s_k - s_{k-1}|.  Bounds: the project's parity bounds (1e-10 fp64, 1e-4 fp32,
relative, on vectors whose maximum is 1) applied to each of the two vectors of a difference:
2e-10 and 2e-4 absolute.

Shapes: 300 ops (the last k_tr_a block finishes the iteration, N <= 512; one ragged k_resid block),
600 ops in a batch of two (the plain call takes pf launches there, the convergence call must not),
17000 ops (N > 16384; four whole k_resid blocks with 16-byte loads and a ragged fifth).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from gpu_util import general_graph, graph_dicts, host_graph_from_oracle

pytestmark = pytest.mark.gpu

ATOL64 = 2e-10
ATOL32 = 2e-4


def oracle_history(g, anomaly, K, precision="fp64"):
    ft = np.float64 if precision == "fp64" else np.float32
    v = orc.preference(g, orc.trace_kinds(g), anomaly)
    prev = (np.ones(g.N) / float(g.N + g.T)).astype(ft).astype(np.float64)
    out = np.empty(K)
    for k in range(1, K + 1):
        s = orc.power_iteration(g, v, iters=k, precision=precision)
        out[k - 1] = np.max(np.abs(s - prev))
        prev = s
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def small():
    g = general_graph(300, 1500, 5)
    return g, host_graph_from_oracle(g)


@functools.lru_cache(maxsize=None)
def small_history(anomaly, K, precision="fp64"):
    return oracle_history(small()[0], anomaly, K, precision)


def upload(hg):
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    return DeviceGraph.upload(_lib.default_context(), hg)


def show(what, got, want):
    err = np.abs(got - want)
    print(f"{what}: max |gpu - oracle| {err.max():.3e} at k={int(err.argmax()) + 1}; "
          f"oracle first {want[0]:.3e} last {want[-1]:.3e}")
    return err


@pytest.mark.parametrize("anomaly", [False, True])
def test_history_against_oracle_last_block_finish(anomaly):
    g, hg = small()
    assert hg.N <= 512
    want = small_history(anomaly, 30)
    dg = upload(hg)
    rep = dg.converge(anomaly, tol=0.0, max_iters=30)
    dg.close()
    err = show(f"300 ops anomaly={anomaly}", rep["residuals"], want)
    assert rep["iters"] == 30 and rep["residuals"].shape == (30,)
    assert rep["converged_at"] is None
    assert (err <= ATOL64).all()


def test_early_stop_at_a_check():
    g, hg = small()
    tol, every = 1e-8, 5
    want = small_history(False, 30)
    at_checks = want[every - 1:20:every]   # k = 5, 10, 15, 20
    print("oracle residuals at the checks:", at_checks)
    assert ((at_checks > 10 * tol) | (at_checks < tol / 10)).all(), "a check sits too close to tol to pin the stop"
    stop = next(k for k in range(every, 31, every) if want[k - 1] <= tol)
    first = int(np.argmax(want <= tol)) + 1
    assert stop == 20 and first <= stop
    dg = upload(hg)
    lib_rep = _raw(dg, False, tol=tol, check_every=every, max_iters=100)
    dg.close()
    assert lib_rep["iters"] == stop
    assert lib_rep["converged_at"] == first
    assert (lib_rep["resid"][stop:] == 0.0).all() and (lib_rep["resid"][:stop] > 0.0).all()
    assert (show("early stop", lib_rep["resid"][:stop], want[:stop]) <= ATOL64).all()


def _raw(dg, anomaly, *, tol, check_every, max_iters, flags=0, expect=None):
    """One graph through the C entry itself: the whole [max_iters] history, or the status when `expect`."""
    from microrank_amd import _lib

    lib = _lib.load()
    hs = (_lib.P * 1)(dg.h)
    an = (C.c_int * 1)(int(anomaly))
    done, conv = C.c_int32(-7), C.c_int32(-7)
    resid = np.full(max(max_iters, 1), -1.0)
    rc = lib.mr_pagerank_converge(dg.ctx.h, hs, an, 1, 0.85, 0.01, max_iters, 0.5, _lib.MR_FP64, flags, tol,
                                  check_every, C.byref(done), resid.ctypes.data_as(_lib.f64p), C.byref(conv))
    if expect is not None:
        assert rc == expect
        return rc
    dg.ctx.check(rc, "mr_pagerank_converge")
    return {"iters": done.value, "converged_at": conv.value, "resid": resid}


def _batch_plain(ctx, dgs, anomaly, iters):
    from microrank_amd import _lib

    hs = (_lib.P * len(dgs))(*[dg.h for dg in dgs])
    an = (C.c_int * len(dgs))(*[int(a) for a in anomaly])
    ctx.check(_lib.load().mr_pagerank_batch(ctx.h, hs, an, len(dgs), 0.85, 0.01, iters, _lib.MR_FP64, 0),
              "mr_pagerank_batch")


def test_bitwise_contract_batch_and_single():
    from microrank_amd import _lib
    from microrank_amd.graph import converge_batch

    hgs = [host_graph_from_oracle(general_graph(600, 3000, s, pr_frac=None, empty_frac=0, rs_drop=0, rs_add=0))
           for s in (5, 6)]
    assert all(512 < hg.N <= 1024 and hg.rs_off is None for hg in hgs)   # fused, past the last-block finish
    anomaly = [False, True]
    ctx = _lib.default_context()
    dgs = [upload(hg) for hg in hgs]
    reps = converge_batch(ctx, dgs, anomaly, tol=1e-6, check_every=5, max_iters=100)
    K = reps[0]["iters"]
    print(f"batch of two 600-op graphs: stopped at {K}, converged_at {[r['converged_at'] for r in reps]}, "
          f"last residuals {[float(r['residuals'][-1]) for r in reps]}")
    assert reps[1]["iters"] == K and 1 <= K <= 100 and K % 5 == 0
    if K < 100:   # stopped at a check: every graph is there, and was not at the check before
        assert all(r["residuals"][K - 1] <= 1e-6 for r in reps)
        assert K == 5 or any(r["residuals"][K - 6] > 1e-6 for r in reps)
    got = [dg.fetch() for dg in dgs]
    fresh = [upload(hg) for hg in hgs]
    _batch_plain(ctx, fresh, anomaly, K)
    for i, (dg, (w, cov)) in enumerate(zip(fresh, got)):
        w_ref, cov_ref = dg.fetch()
        assert np.all(np.isfinite(w_ref)) and np.any(w_ref != 0)
        print(f"batch graph {i}: weights byte-equal: {w.tobytes() == w_ref.tobytes()}")
        np.testing.assert_array_equal(w, w_ref)
        np.testing.assert_array_equal(cov, cov_ref)
    # one graph alone
    rep = dgs[0].converge(False, tol=1e-6, check_every=5, max_iters=100)
    w, cov = dgs[0].fetch()
    fresh[0].pagerank(False, iters=rep["iters"])
    w_ref, cov_ref = fresh[0].fetch()
    print(f"single graph: stopped at {rep['iters']}, weights byte-equal: {w.tobytes() == w_ref.tobytes()}")
    np.testing.assert_array_equal(w, w_ref)
    np.testing.assert_array_equal(cov, cov_ref)
    for dg in dgs + fresh:
        dg.close()


def test_wide_graph_reports_non_convergence():
    g = general_graph(17000, 3000, 5, mean_len=6)
    hg = host_graph_from_oracle(g)
    assert hg.N > 16384
    want = oracle_history(g, False, 12)
    print("oracle history:", want)
    assert (want > 1e-6).all()
    dg = upload(hg)
    rep = dg.converge(False, tol=1e-9, max_iters=12, check_every=4)
    dg.close()
    err = show("17000 ops", rep["residuals"], want)
    assert rep["iters"] == 12 and rep["converged_at"] is None
    assert (err <= ATOL64).all()


def test_fp32_history():
    g, hg = small()
    want = small_history(False, 20, "fp32")
    dg = upload(hg)
    rep = dg.converge(False, tol=0.0, max_iters=20, precision="fp32")
    dg.close()
    err = show("300 ops fp32", rep["residuals"], want)
    assert rep["iters"] == 20
    assert (err <= ATOL32).all()


def test_rerun_is_bitwise():
    g, hg = small()
    dg = upload(hg)
    a = dg.converge(False, tol=0.0, max_iters=30)
    b = dg.converge(False, tol=0.0, max_iters=30)
    dg.close()
    assert a["iters"] == b["iters"] == 30
    assert a["residuals"].tobytes() == b["residuals"].tobytes()


def test_collision_retry_overwrites_the_history(monkeypatch):
    """MR_KIND_TEST_COLLIDE makes the first attempt's kind keys collide: the attempt reruns with the
    next seed and the report is the uncollided call's, bit for bit (weights too)."""
    g, hg = small()
    dg = upload(hg)
    base = _raw(dg, True, tol=1e-8, check_every=5, max_iters=60)
    w_base = dg.fetch()[0]
    monkeypatch.setenv("MR_KIND_TEST_COLLIDE", "1")
    coll = _raw(dg, True, tol=1e-8, check_every=5, max_iters=60)
    monkeypatch.delenv("MR_KIND_TEST_COLLIDE")
    w_coll = dg.fetch()[0]
    dg.close()
    assert 0 < base["iters"] < 60
    assert (coll["iters"], coll["converged_at"]) == (base["iters"], base["converged_at"])
    assert coll["resid"].tobytes() == base["resid"].tobytes()
    assert w_coll.tobytes() == w_base.tobytes()


def test_rejected_arguments_leave_the_graph_usable():
    from microrank_amd import _lib

    g, hg = small()
    dg = upload(hg)
    ok = dict(tol=1e-8, check_every=5, max_iters=10)
    for bad in (dict(flags=_lib.MR_PR_KIND_COMPRESS), dict(check_every=0), dict(tol=-1.0), dict(tol=float("nan")),
                dict(max_iters=0)):
        rc = _raw(dg, False, **{**ok, **bad}, expect=_lib.MR_ERR_ARG)
        with pytest.raises(ValueError):
            dg.ctx.check(rc, "mr_pagerank_converge")
    with pytest.raises(ValueError):
        dg.converge(False, tol=-1.0)
    with pytest.raises(ValueError):
        dg.converge(False, tol=1e-8, check_every=0)
    v = orc.preference(g, orc.trace_kinds(g), False)
    w_ref = np.array(list(orc.weights(g, orc.power_iteration(g, v))[0].values()))
    dg.pagerank(False)
    w, _ = dg.fetch()
    dg.close()
    assert ((w == 0) == (w_ref == 0)).all()
    np.testing.assert_allclose(w, w_ref, rtol=1e-10, atol=0)


def test_trace_pagerank_to_a_tolerance():
    from microrank_amd.pagerank import trace_pagerank

    dicts = graph_dicts(small()[0])
    info = {}
    w, num = trace_pagerank(*dicts, False, tol=1e-8, info=info)
    assert set(info) == {"iters", "residuals", "converged_at"}
    want = small_history(False, 30)
    first = int(np.argmax(want <= 1e-8)) + 1
    assert info["iters"] == 20 and info["converged_at"] == first and info["residuals"].shape == (20,)
    assert (np.abs(info["residuals"] - want[:20]) <= ATOL64).all()
    w_fix, num_fix = trace_pagerank(*dicts, False, iters=info["iters"])
    assert list(w) == list(w_fix) and num == num_fix
    assert np.array(list(w.values())).tobytes() == np.array(list(w_fix.values())).tobytes()
