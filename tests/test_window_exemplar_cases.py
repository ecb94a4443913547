"""The properties the window-batch exemplar tests rest on, asserted on the CPU with the oracle
(window_exemplar_cases): a drifting generator fails here, not in a GPU test's margin.

  ragged      65 abnormal traces (one full wave tile + a tile of one trace), 65 normal; the abnormal
              traces' graph has 30 ops, every top op is a node of it, coverages 5..65, and the op of
              coverage 33 has an exact oracle tie at the m = 32 cut
  one_trace   exactly 1 abnormal trace, 129 normal; the abnormal traces' graph has 5 ops and 1 trace,
              so most of the top list is ABSENT from it (the case with absent top ops)
  mid         500 abnormal (500 mod 64 = 52), 294 ops, top of 11, coverages 37..500
  ties        1000 abnormal traces with only 189 distinct oracle r values; 14 exact ties inside the
              top 32 of the most covered op
  span_times  300 / 300; times vary within a trace (the window takes the per-span-time route)
"""
import inspect

import numpy as np
import pytest

import window_exemplar_cases as wc


def _cov(name):
    return np.array(sorted(wc.coverage(name).values()))


def test_ragged():
    o = wc.oracle("ragged", 25)
    assert (o.n_abnormal, o.n_normal, o.N, o.T) == (65, 65, 30, 65) and len(o.top) == wc.K_TOP
    cov = _cov("ragged")
    assert cov.min() == 5 and cov.max() == 65 and (cov > 0).all()
    (code,) = [c for c, n in wc.coverage("ragged").items() if n == 33]
    v = np.sort(o.r[o.rows[code]])[::-1]
    assert v[31] == v[32], "no exact tie at the m = 32 cut"


def test_one_trace():
    o = wc.oracle("one_trace", 25)
    assert (o.n_abnormal, o.n_normal, o.N, o.T) == (1, 129, 5, 1) and len(o.top) == wc.K_TOP
    cov = wc.coverage("one_trace")
    assert any(n == 0 for n in cov.values()) and any(n == 1 for n in cov.values())
    assert all(c not in o.rows for c, n in cov.items() if n == 0)


def test_mid():
    o = wc.oracle("mid", 25)
    assert (o.n_abnormal, o.n_normal, o.N, o.T) == (500, 500, 294, 500) and o.T % 64 == 52 and len(o.top) == wc.K_TOP
    cov = _cov("mid")
    assert cov.min() == 37 and cov.max() == 500


def test_ties():
    o = wc.oracle("ties", 25)
    assert (o.n_abnormal, o.T) == (1000, 1000) and np.unique(o.r).size == 189
    cov = wc.coverage("ties")
    top = max(cov, key=cov.get)
    v = np.sort(o.r[o.rows[top]])[::-1][:32]
    assert int((np.diff(v) == 0).sum()) == 14


def test_span_times():
    st = wc.table("span_times")[0]
    o = wc.oracle("span_times", 25)
    assert (o.n_abnormal, o.n_normal) == (300, 300)
    lo = np.full(st.n_traces, np.iinfo(np.int64).max)
    hi = np.full(st.n_traces, np.iinfo(np.int64).min)
    np.minimum.at(lo, st.trace, st.tstart)
    np.maximum.at(hi, st.trace, st.tstart)
    assert (hi > lo).any(), "start times do not vary within a trace"


def test_coverages_straddle_m():
    """m = 32 cuts rows (coverage > 32) in mid and in ragged and leaves rows short (coverage < 32) in
    ragged and span_times.  mid's smallest top coverage is 37 (asserted above), so mid itself has no
    short row at m = 32."""
    mid, ragged = _cov("mid"), _cov("ragged")
    assert (mid > 32).any() and (ragged > 32).any()
    assert ((ragged > 0) & (ragged < 32)).any()
    assert ((_cov("span_times") > 0) & (_cov("span_times") < 32)).any()   # ... and span_times' (26, 26)


def test_some_top_op_is_absent_from_the_abnormal_graph():
    assert any(n == 0 for name in wc.NAMES for n in wc.coverage(name).values())


@pytest.mark.parametrize("name", wc.NAMES)
def test_fp32_iteration_count_has_the_same_nodes(name):
    """The fp32 legs rank with 7 iterations: same graph, so the same rows; the top list exists."""
    o = wc.oracle(name, wc.ITERS["fp32"])
    assert len(o.top) == wc.K_TOP and o.T == wc.oracle(name, 25).T


def test_new_surface():
    from microrank_amd import _lib, online_rca

    assert "mr_windows_batch_exemplars" in _lib.SIGNATURES
    assert inspect.signature(online_rca.rank_windows).parameters["exemplars"].default is None
