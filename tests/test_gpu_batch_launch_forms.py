"""One mr_pagerank_batch call gives the same weights whichever launch form its iterations take:
the last k_tr_a block finishing each graph (default), the next launch's blocks finishing it
(MR_TR_LASTFIN=0: the pf launches), k_fx_b every iteration (MR_TR_PF=0), k_fx_b computing the
call-graph terms itself (MR_TR_SSV=0), and the last block reading the terms through the chain
(MR_TR_LFSSV=0) -- and the default form gives what each graph's own ranking gives.

The three graphs of test_gpu_setup_paths (T = 1, 255, 300; 40 ops): three graphs in one call, so
the blocks find their graph by search (no two-graph split).

Every pair is compared byte for byte: the knobs only choose which block sums the same fixed-point
integers, and a graph's blocks and scale do not depend on the batch around it.  All of them were
byte-equal on the commit before this test was added (the rtol 1e-12 that test_gpu_setup_paths allows
batched against per-graph weights was not needed for any pair).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_setup_paths import ANOMALY, TRACES, host_graphs  # noqa: F401  (the same three graphs)

pytestmark = pytest.mark.gpu

KNOBS = ("MR_TR_LASTFIN", "MR_TR_PF", "MR_TR_SSV", "MR_TR_LFSSV", "MR_TR_ROW_WT", "MR_NO_SETUP_BATCH")
FORMS = {
    "default": {},
    "pf": {"MR_TR_LASTFIN": "0"},
    "fx_b": {"MR_TR_LASTFIN": "0", "MR_TR_PF": "0"},
    "fx_b_no_ssv": {"MR_TR_LASTFIN": "0", "MR_TR_PF": "0", "MR_TR_SSV": "0"},
    "lf_chain": {"MR_TR_LFSSV": "0"},
}


def _rank_batch(ctx, dgs, precision, monkeypatch, form):
    """The weights of one mr_pagerank_batch call over dgs under a form's knobs (read per call)."""
    from microrank_amd import _lib

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    lib = _lib.load()
    hs = (_lib.P * len(dgs))(*[dg.h for dg in dgs])
    an = (C.c_int * len(dgs))(*ANOMALY)
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    rc = lib.mr_pagerank_batch(ctx.h, hs, an, len(dgs), 0.85, 0.01, 25, prec, 0)
    for k in FORMS[form]:
        monkeypatch.delenv(k)
    assert rc == _lib.MR_OK
    return [dg.fetch()[0] for dg in dgs]


def _compare(pair, got, want):
    """Every graph of a pair byte for byte: prints each one's result, returns the misses."""
    missed = []
    for T, g, w in zip(TRACES, got, want):
        eq = g.tobytes() == w.tobytes()
        print(f"{pair} T={T}: byte-equal: {eq}")
        assert np.all(np.isfinite(w)) and np.any(w != 0)
        if not eq:
            rel = float(np.max(np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)))
            missed.append(f"{pair} T={T}: not byte-equal, max rel {rel:.3e}")
    return missed


@pytest.fixture(scope="module")
def device_graphs(host_graphs):  # noqa: F811
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    ctx = _lib.default_context()
    dgs = [DeviceGraph.upload(ctx, hg) for hg in host_graphs]
    yield ctx, dgs
    for dg in dgs:
        dg.close()


def test_fp64_launch_forms_give_the_default_forms_weights(device_graphs, monkeypatch):
    ctx, dgs = device_graphs
    want = _rank_batch(ctx, dgs, "fp64", monkeypatch, "default")
    got = {form: _rank_batch(ctx, dgs, "fp64", monkeypatch, form) for form in FORMS if form != "default"}
    missed = [m for form, w in got.items() for m in _compare(form, w, want)]
    assert not missed, missed


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_default_form_gives_each_graphs_own_ranking(device_graphs, precision, monkeypatch):
    ctx, dgs = device_graphs
    batched = _rank_batch(ctx, dgs, precision, monkeypatch, "default")
    alone = []
    for dg, a in zip(dgs, ANOMALY):
        dg.pagerank(bool(a), precision=precision)   # (raises unless MR_OK)
        alone.append(dg.fetch()[0])
    missed = _compare(f"alone/{precision}", batched, alone)
    assert not missed, missed
