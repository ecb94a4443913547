"""The cases of tests/wide_cases.py keep the shapes the wide-graph batch tests rest on: built on the
CPU, no GPU needed.  A generator change that turns one of them narrow (or moves it off the path it
stands for) fails here, not silently on the GPU."""
import numpy as np
import pytest

import oracle as orc
import wide_cases as wc


def test_w1_is_wide_with_one_cold_range():
    s = wc.case("W1").shape
    print(vars(s))
    assert s.N > wc.FX_NMAX and s.wide
    assert s.cold_entries >= 10000
    assert s.cold_ranges == 1 and s.N - wc.WIDE_NA <= wc.WIDE_RW_MAX


def test_w2_has_two_cold_ranges_hotless_traces_and_long_tiles():
    s = wc.case("W2").shape
    print(vars(s))
    assert s.N > wc.FX_NMAX and s.cold_ranges == 2
    assert s.cold_entries >= 60000
    assert s.traces_without_hot > 0
    assert s.max_trace > 32
    # tiles k_cold_trace keeps: traces with more hot ids than the short tiers hold (n_ctl > 0)
    assert s.past_short_hot > 0
    # fp32: cold labels past the warm ones exist (the next ~9.8k labels after the hot ones are warm)
    assert s.N - wc.WIDE_NA > 2 * 9800


def test_narrow_cases_sit_on_their_side_of_the_su_in_lds_limit():
    n1, n2 = wc.case("N1").shape, wc.case("N2").shape
    assert not n1.wide and n1.su_in_lds and not n1.tile_path
    assert not n2.wide and not n2.su_in_lds and not n2.tile_path
    assert wc.SU_LDS_NMAX < n2.N <= wc.FX_NMAX
    assert (n2.N + 64) * 16 > 160 * 1024 - 512


def test_tp_is_on_the_tile_path():
    c = wc.case("TP")
    assert c.shape.tile_path and c.hg.rs_off is not None


def test_wk_repeats_kinds_and_stays_wide():
    c = wc.case("WK")
    n_kinds = float((1.0 / c.kind).sum())
    print(f"WK: {n_kinds:.0f} kinds of {c.hg.T} traces")
    assert c.shape.N > wc.FX_NMAX and c.shape.wide
    assert abs(n_kinds - round(n_kinds)) < 1e-6 * n_kinds
    assert round(n_kinds) <= 0.55 * c.hg.T
    w1 = wc.case("W1")
    assert c.hg.T == 2 * w1.hg.T and int(c.hg.sr_off[-1]) == c.hg.sr_ops.size > w1.hg.sr_ops.size
    # a repeated trace is the same row again, so the kinds of its copies are one kind
    assert np.array_equal(c.hg.sr_ops[c.hg.sr_off[1]:c.hg.sr_off[2]], c.hg.sr_ops[c.hg.sr_off[2]:c.hg.sr_off[3]])
    assert (np.bincount(c.hg.sr_ops, minlength=c.hg.N) <= c.hg.len_o).all()


@pytest.mark.parametrize("name", wc.WINDOWS)
def test_window_cases_split_as_stated(name):
    na, nn, (g_ab, g_no) = wc.window_graphs(name)
    print(f"{name}: {na} abnormal / {nn} normal traces, N = {g_ab.N} / {g_no.N}")
    assert na > 0 and nn > 0
    assert g_no.N > wc.FX_NMAX
    if name == "WS":
        assert g_ab.N > wc.FX_NMAX
    else:   # narrow, fused (a span graph's P_rs is P_sr's transpose), su out of LDS
        assert wc.SU_LDS_NMAX < g_ab.N <= wc.FX_NMAX
    assert g_ab.ss_c.size > 0 and g_no.ss_c.size > 0


def test_converge_case_stops_at_its_second_check():
    """The converge test's early stop, pinned on the oracle's histories (wide_cases.converge_stop
    asserts the margins): W1 reaches the tolerance before the call's maximum, the batch at K = 6."""
    K, first = wc.converge_stop()
    for (n, a), f in zip(wc.CONVERGE_BATCH, first):
        print(n, a, "converged_at", f, wc.history(n, a, wc.CONVERGE_MAX))
    assert K == 2 * wc.CONVERGE_EVERY
    assert first[0] < K < wc.CONVERGE_MAX and max(first) <= K
