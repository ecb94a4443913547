"""mr_pagerank_sharded_converge on the GPU: ranks that share one GPU (host collectives over gloo unless
said otherwise) rank the window graph of tests/test_dist_gloo.py to a tolerance.  The history is the
WHOLE graph's residual (the CPU oracle's max|s_k - s_{k-1}|, DESIGN §7's 2e-10), byte-equal on every
rank; the ranks stop at the same check, the one the oracle names (its residuals at the checks: 1.30e-8
at 40 and 9.99e-10 at 45 for the normal preference, 1.58e-8 at 25 and 7.1e-10 at 30 for the anomaly
preference, so tol = 3e-9 has a factor >= 3 on both sides); the weights are byte-equal to
mr_pagerank_sharded with that count in the same processes.  Several checks share each spawned run."""
import numpy as np
import pytest

from shard_evidence_util import (CHECK, TOL, expected_stop, oracle_history, run, span_run, whole_graph)

pytestmark = pytest.mark.gpu

MR_ERR_ARG = 1


@pytest.fixture(scope="module")
def two():
    return run(2, "converge", fp32=True, errors=True)


@pytest.mark.parametrize("anomaly", [False, True])
def test_history_is_the_whole_graphs_and_equal_on_every_rank(two, anomaly):
    ref = oracle_history(anomaly)
    for res in two:
        o = res[anomaly]
        assert o["hist_iters"] == 60 and o["hist"].shape == (60,)
        print("history: max |gpu - oracle| =", np.max(np.abs(o["hist"] - ref)))
        np.testing.assert_allclose(o["hist"], ref, rtol=0, atol=2e-10)
        assert o["hist_w_same"], "weights differ from sharded_pagerank(iters=60)"
        assert o["hist_conv"] is None or o["hist"][o["hist_conv"] - 1] == 0.0   # (tol = 0)
    assert two[0][anomaly]["hist"].tobytes() == two[1][anomaly]["hist"].tobytes(), "ranks disagree"


def _check_stop(results, anomaly, w_rtol):
    k = expected_stop(anomaly)
    w_ref, cov_ref, _ = whole_graph(anomaly, k)
    for res in results:
        o = res[anomaly]
        assert o["stop"] == k, (o["stop"], k)
        assert o["stop_w_same"], "weights differ from sharded_pagerank(iters=stop)"
        h = o["stop_hist"]
        assert h.shape == (k,)
        assert o["stop_conv"] == next(i + 1 for i in range(k) if h[i] <= TOL)
        np.testing.assert_allclose(o["w"], w_ref, rtol=w_rtol, atol=0)
        np.testing.assert_array_equal(o["cov"], cov_ref)
    for res in results[1:]:
        assert res[anomaly]["w"].tobytes() == results[0][anomaly]["w"].tobytes(), "ranks disagree"
        assert res[anomaly]["stop_hist"].tobytes() == results[0][anomaly]["stop_hist"].tobytes(), "ranks disagree"


@pytest.mark.parametrize("anomaly", [False, True])
def test_stop_at_the_oracles_check(two, anomaly):
    assert expected_stop(anomaly) == (30 if anomaly else 45)
    assert CHECK == 5
    _check_stop(two, anomaly, 1e-12)


@pytest.mark.parametrize("form", ["peer", "tile"])
def test_four_ranks_stop_with_the_two(form):
    """peer: the per-iteration exchange through the peer regions (the checks' words still go through the
    fallback collective); tile: MR_NO_FUSED, fp64 per-op sums."""
    res = run(4, "converge", history=False, peer=form == "peer", tile=form == "tile")
    for anomaly in (False, True):
        _check_stop(res, anomaly, 1e-10 if form == "tile" else 1e-12)


def test_empty_rank_joins_every_check():
    res = run(2, "converge", history=False, cut="empty_last")
    assert res[1]["T"] == 0
    for anomaly in (False, True):
        _check_stop(res, anomaly, 1e-10)


@pytest.mark.parametrize("anomaly", [False, True])
def test_fp32_history(two, anomaly):
    ref = oracle_history(anomaly)[:30]
    for res in two:
        h = res[anomaly]["hist32"]
        print("fp32 history: max |gpu - oracle| =", np.max(np.abs(h - ref)))
        np.testing.assert_allclose(h, ref, rtol=0, atol=2e-4)
    assert two[0][anomaly]["hist32"].tobytes() == two[1][anomaly]["hist32"].tobytes()


def test_one_rank_rccl():
    res = run(1, "converge", history=False, backend="rccl")
    for anomaly in (False, True):
        _check_stop(res, anomaly, 1e-12)


def test_differing_requests_fail_on_every_rank_and_the_next_call_works(two):
    for res in two:
        e = res["errors"]
        assert e["disagree"].startswith("ValueError") and "differs" in e["disagree"], e["disagree"]
        assert e["after"] == expected_stop(True)
        assert e["kind_compress"] == MR_ERR_ARG


def test_mr_pagerank_converge_still_rejects_a_built_shard():
    for res in span_run():
        assert res["old_converge"].startswith("ValueError") and "mr_graph_build_sharded" in res["old_converge"]
        assert res["stop_w_same"] and res["stop"] >= CHECK and res["stop"] % CHECK == 0
    assert span_run()[0]["stop"] == span_run()[1]["stop"]
