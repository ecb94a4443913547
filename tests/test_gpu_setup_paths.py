"""The PageRank set-up (reset + iteration state, kinds, preference) gives the same kinds and
preference whichever of its forms runs: batched over the graphs of one mr_pagerank_batch call,
per graph inside that call (MR_NO_SETUP_BATCH), or a graph's own ranking.

Three small graphs of T = 1, 255 and 300 traces: a single trace, one short block, and one block
plus a remainder of the set-up's 256-thread blocks.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from gpu_util import host_graph_from_oracle

pytestmark = pytest.mark.gpu

TRACES = (1, 255, 300)
ANOMALY = (0, 1, 1)


@pytest.fixture(scope="module")
def host_graphs():
    from microrank_amd import synth

    topo = synth.make_topology(40, 3)
    out = []
    for T in TRACES:
        st = synth.gen_spans(topo, T, 4, branch=4.0, p_max=0.7, names=False)
        sg = orc.span_graph(st.trace, st.podop, st.span, st.parent, np.ones(st.n_traces, dtype=bool))
        out.append(host_graph_from_oracle(sg.as_graph()))
    assert [hg.T for hg in out] == list(TRACES)
    return out


def _rank_batch(ctx, dgs, precision):
    """One mr_pagerank_batch call over dgs (the driver's d, alpha and 25 iterations)."""
    from microrank_amd import _lib

    lib = _lib.load()
    hs = (_lib.P * len(dgs))(*[dg.h for dg in dgs])
    an = (C.c_int * len(dgs))(*ANOMALY)
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    rc = lib.mr_pagerank_batch(ctx.h, hs, an, len(dgs), 0.85, 0.01, 25, prec, 0)
    assert rc == _lib.MR_OK
    return [dg.fetch(kinds=True) for dg in dgs]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_setup_forms_give_the_same_kinds_and_preference(host_graphs, precision, monkeypatch):
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    ctx = _lib.default_context()
    dgs = [DeviceGraph.upload(ctx, hg) for hg in host_graphs]
    monkeypatch.delenv("MR_NO_SETUP_BATCH", raising=False)
    batched = _rank_batch(ctx, dgs, precision)
    monkeypatch.setenv("MR_NO_SETUP_BATCH", "1")
    per_graph = _rank_batch(ctx, dgs, precision)
    monkeypatch.delenv("MR_NO_SETUP_BATCH")
    for (w_a, _, k_a, p_a), (w_b, _, k_b, p_b) in zip(batched, per_graph):
        # kinds are integer counts; both preference forms evaluate one expression on sums of one shape
        assert k_a.tobytes() == k_b.tobytes()
        assert p_a.tobytes() == p_b.tobytes()
        print(f"T={k_a.size} {precision}: weights batched vs per-graph byte-equal: {w_a.tobytes() == w_b.tobytes()}")
        np.testing.assert_allclose(w_a, w_b, rtol=1e-12, atol=0)
    for dg, a, (_, _, k_a, p_a) in zip(dgs, ANOMALY, batched):
        dg.pagerank(bool(a), precision=precision)   # (raises unless MR_OK)
        _, _, k_c, p_c = dg.fetch(kinds=True)
        assert k_a.tobytes() == k_c.tobytes()
        assert p_a.tobytes() == p_c.tobytes()
    for dg in dgs:
        dg.close()


def test_kind_compressed_set_up_matches_uncompressed(host_graphs):
    """The kind-compressed ranking (its own reset launch, multiplicities in the preference sums)
    against the plain one on the largest graph: same kinds, weights within 1e-10."""
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    ctx = _lib.default_context()
    dg = DeviceGraph.upload(ctx, host_graphs[-1])
    dg.pagerank(True)
    w0, _, k0, _ = dg.fetch(kinds=True)
    dg.pagerank(True, compress_kinds=True)
    w1, _, k1, _ = dg.fetch(kinds=True)
    np.testing.assert_array_equal(k1, k0)
    np.testing.assert_allclose(w1, w0, rtol=1e-10, atol=0)
    dg.close()
