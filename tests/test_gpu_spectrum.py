"""Stand-alone K3 (mr_spectrum: k_spectrum, the one-block bitonic sort up to 4096 nodes, the 64-bit
radix sort above, k_gather_top) against the numpy oracle on the generated inputs of
tests/spectrum_cases.py -- all 13 formulas, both sorts, the sizes around the powers of two and
the sort switch, exact-tie groups of hundreds of nodes, -0.0 / +0.0 / inf scores, Python and numpy
typed weights, and a zero division flagged by the union's last node.  Every comparison is bitwise:
the kernel performs the reference's operations in the reference's order, and the oracle is pinned
to the reference on these inputs by tests/golden/spectrum_synth.json (test_oracle_golden.py)."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import spectrum_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu

# mr_sort.hip: the radix sort runs above SL_MAX = 4096 keys (mr_spectrum.hip: SB = 4096) in tiles of
# RTILE = RT * RC = 256 * 8 = 2048 keys, a block per tile.  So the smallest n with more than one block
# per pass and a partial last tile is SL_MAX + 1 = 2 * RTILE + 1 = 4097 itself (three blocks, the last
# with one key).  2 * RTILE + RT + 1 = 4353 adds the case 4097 and 4099 leave out: a last tile of one
# full chunk of RT keys and a chunk of one key, so the tile's running digit offsets carry from a
# chunk into a partial one.
RADIX_TILE, RADIX_CHUNK = 2048, 256
SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 4099,
         2 * RADIX_TILE + RADIX_CHUNK + 1, 20011]
FIXTURE_SIZES = (1, 2, 3, 65, 1025, 4097)


def _spec(case, method, top_max):
    """The Python surface: (top, score, printed text)."""
    from microrank_amd.online_rca import calculate_spectrum_without_delay_list as spec

    a, nr, an, nn, A, N = case
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        top, score = spec(anomaly_result=a, normal_result=nr, anomaly_list_len=A, normal_list_len=N, top_max=top_max,
                          normal_num_list=nn, anomaly_num_list=an, spectrum_method=method)
    return top, score, buf.getvalue()


def _hex(scores):
    return [float(s).hex() for s in scores]


def _check_full(case, method, exp, where):
    n = len(sc.union(case))
    top, score, text = _spec(case, method, n - 6)
    e_top, e_score, e_lines = exp
    assert len(top) == len(score) == n, where
    assert top == e_top, where                                   # the stable order through every tie group
    assert _hex(score) == _hex(e_score), where                   # -0.0 keeps its sign, inf is inf
    assert [type(s) for s in score] == [type(s) for s in e_score], where
    assert text == "".join(ln + "\n" for ln in e_lines), where
    return top, score


@pytest.fixture(scope="module")
def synth_fixture():
    fix = load_golden("spectrum_synth.json")
    return {(c["n"], c["typed"]): c["out"] for c in fix["cases"]}


@pytest.mark.parametrize("typed", ["np", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_spectrum_full_list_all_methods(n, typed, synth_fixture):
    """Every method's whole sorted list (top_max = n - 6): names, score bits, score types and the
    printed lines equal the oracle's; at the fixture's sizes the first 11 equal the reference's
    recorded ones too."""
    exp = sc.expected(n, typed)
    for m in sc.METHODS:
        top, score = _check_full(sc.case_for(m, n, typed=typed), m, exp[m], (n, typed, m))
        if n in FIXTURE_SIZES:
            rec = synth_fixture[(n, typed)][m]
            assert top[:11] == rec["top"] and _hex(score[:11]) == rec["score"], (n, typed, m)
            assert ["np.float64" if isinstance(s, np.float64) else type(s).__name__ for s in score[:11]] == rec["type"]


@pytest.mark.parametrize("n", [5, 4096, 4097, 20011])
def test_spectrum_zero_division_from_last_node(n):
    """"zd_last": the union's last node (the last thread of k_spectrum's last block) is all-Python
    with ep + nf == 0.  ZeroDivisionError for exactly the methods the oracle raises for (dstar2,
    m1); the other methods return the oracle's list bitwise; the call after a raising call on the
    same context succeeds."""
    exp = sc.expected(n, "zd_last")
    assert [m for m in sc.METHODS if exp[m] == "ZeroDivisionError"] == ["dstar2", "m1"]
    for m in sc.METHODS:
        case = sc.case_for(m, n, typed="zd_last")
        if exp[m] == "ZeroDivisionError":
            with pytest.raises(ZeroDivisionError):
                _spec(case, m, n - 6)
            _check_full(sc.case_for("jaccard", n, typed="zd_last"), "jaccard", exp["jaccard"], (n, "after", m))
        else:
            _check_full(case, m, exp[m], (n, "zd_last", m))


def _arrays(case):
    """The C ABI's per-node arrays in union order (membership bit 0, numpy-typed bit 1)."""
    a, nr, an, nn, _, _ = case
    nodes = sc.union(case)
    n = len(nodes)
    has_a, has_n = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    a_w, n_w = np.zeros(n, np.float64), np.zeros(n, np.float64)
    a_num, n_num = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i, k in enumerate(nodes):
        if k in a:
            a_w[i], a_num[i] = a[k], an[k]
            has_a[i] = 1 | (2 if isinstance(a[k], np.generic) else 0)
        if k in nr:
            n_w[i], n_num[i] = nr[k], nn[k]
            has_n[i] = 1 | (2 if isinstance(nr[k], np.generic) else 0)
    return nodes, has_a, a_w, a_num, has_n, n_w, n_num


@pytest.mark.parametrize("n", [3, 4097])
def test_spectrum_top_through_c_abi(n):
    """mr_spectrum's ``top``: *n_out == min(n, max(top, 0)), the entries are the prefix of the full
    list, and the output buffers past n_out keep their sentinel."""
    from microrank_amd import _lib
    from microrank_amd._lib import SPECTRUM_METHODS, ptr

    ctx = _lib.default_context()
    m = "jaccard"
    case = sc.case_for(m, n)
    e_top, e_score, _ = sc.expected(n, "np")[m]
    nodes, has_a, a_w, a_num, has_n, n_w, n_num = _arrays(case)
    pad = 16
    for top in (-2, 0, 1, n - 1, n, n + 5):
        idx = np.full(n + pad, -77, np.int32)
        score = np.full(n + pad, -12345.5, np.float64)
        n_out, zd = C.c_int32(-1), C.c_int32(-1)
        ctx.check(_lib.load().mr_spectrum(ctx.h, n, ptr(has_a, C.c_uint8), ptr(a_w, C.c_double), ptr(a_num, C.c_int64),
                                          ptr(has_n, C.c_uint8), ptr(n_w, C.c_double), ptr(n_num, C.c_int64), case[4],
                                          case[5], SPECTRUM_METHODS.index(m), top, ptr(idx, C.c_int32),
                                          ptr(score, C.c_double), C.byref(n_out), C.byref(zd)), "mr_spectrum")
        k = min(n, max(top, 0))
        assert n_out.value == k and zd.value == 0, top
        assert [nodes[i] for i in idx[:k]] == e_top[:k], top
        assert _hex(score[:k]) == _hex(e_score[:k]), top
        assert (idx[k:] == -77).all() and (score[k:] == -12345.5).all(), top


def test_spectrum_is_deterministic():
    """The n = 4097 "np" dstar2 call (radix route, tie groups of hundreds) twice: identical bytes."""
    case = sc.case_for("dstar2", 4097)
    a = _spec(case, "dstar2", 4097 - 6)
    b = _spec(case, "dstar2", 4097 - 6)
    assert a[0] == b[0] and a[2] == b[2]
    assert np.array(a[1], np.float64).tobytes() == np.array(b[1], np.float64).tobytes()
