"""GPU parity of trace_pagerank on general graphs: what any four dicts can hold, not only what
get_pagerank_graph builds -- P_rs that is not the transpose of P_sr, a pr_trace that is a subset
of the traces in its own order with its own lengths, traces without ops, list multiplicities in
len_t / len_o / nchild (gpu_util.general_graph).

A graph uploaded with explicit rs arrays never takes the fused iteration: it runs k_iter_a (trace
role over P_rs, tile role over the P_sr tiles) and k_iter_b, the tile build of mr_graph_prepare,
the int32 kind kernels and the preference kernels with pr_trace / pr_len pointers.  The shapes are
the smallest that reach each regime of those kernels; every case asserts on the host, from the
arrays it uploads, that it does reach it (_regime mirrors the constants of mr_pr_internal.h,
which the tile path's kernels in mr_pr_tile_dev.h read).

Reference: the oracle (fp64 weights 1e-10 on every entry, an exact 0 stays an exact 0; fp32 1e-4;
kinds and coverage exact; the preference bit for bit with exact_sums, within one fp32 ulp with
the tree sums), and for the 300-op / 1500-trace graph the reference's own output as well
(tests/golden/dict_general.json).
"""
import ctypes as C
import dataclasses
import functools
import types

import numpy as np
import pytest

import oracle as orc
from conftest import load_golden, unhex
from gpu_util import general_golden_dicts, general_graph, host_graph_from_oracle

pytestmark = pytest.mark.gpu

RTOL64 = 1e-10     # the tolerances of test_gpu_pagerank
RTOL32 = 1e-4
PREF_ULP = 1.2e-7  # tree vs sequential preference sums: <= 1 fp32 ulp (test_c2_scale_against_oracle)
SEED = 3

# mr_pr_internal.h (k_iter_a / k_iter_b: mr_pr_tile_dev.h): trace-role block, ids staged per round, su in LDS up to,
# wave-per-pair above, u16 ids up to, fused iteration up to
TB, VCAP, LDS_NODES, LONG_PAIR, U16_NODES, FX_NMAX = 256, 2048, 8192, 32, 65536, 16384

#        name              N      T      knobs
CASES = {
    "one_trace":       (300,   1,     dict(empty_frac=0)),
    "ragged_tile":     (300,   200,   {}),
    "six_tiles":       (300,   1536,  {}),
    "long_pairs":      (300,   1500,  {}),                      # the graph of dict_general.json
    "su_global":       (9000,  3000,  dict(long_trace=2500)),
    "int32_ids":       (70000, 1500,  {}),
    "tshift9":         (300,   70000, dict(mean_len=4)),
    "fused_pr_subset": (300,   1500,  dict(rs_drop=0, rs_add=0, empty_frac=0)),
    # rs == sr forms of two graphs above (fused when uploaded as they are, tiles with explicit rs)
    "su_global_rs_is_sr": (9000, 3000, dict(long_trace=2500, rs_drop=0, rs_add=0, empty_frac=0)),
}
FP32_FULL = ("long_pairs",)
FP32_MASKED = ("su_global",)   # ops reached only through the alpha chain sit near 1e-20 there


def _regime(hg):
    """What the uploaded arrays make the tile path do (mr_graph_prepare's tile shape, k_iter_a's rounds)."""
    T, N = hg.T, hg.N
    ts = 8
    while ts < 12 and (T >> ts) > 256:
        ts += 1
    sr_t = np.repeat(np.arange(T, dtype=np.int64), np.diff(hg.sr_off))
    _, per_pair = np.unique((sr_t >> ts) * N + hg.sr_ops, return_counts=True)
    off = hg.rs_off if hg.rs_off is not None else hg.sr_off
    blocks = np.minimum(np.arange(0, T + TB, TB), T)
    return types.SimpleNamespace(tshift=ts, n_tiles=-(-T // (1 << ts)), long_pairs=int((per_pair > LONG_PAIR).sum()),
                                 max_block_ids=int(np.diff(off[blocks]).max()), max_row=int(np.diff(off).max()),
                                 tile_path=hg.rs_off is not None or bool((np.diff(hg.sr_off) == 0).any()))


def _assert_regime(name, hg):
    r = _regime(hg)
    fused = name in ("fused_pr_subset", "su_global_rs_is_sr")
    assert r.tile_path == (not fused), name
    if hg.T > 1:   # pr_trace: a subset of the traces, not in trace order, with lengths of its own
        assert hg.pr_trace is not None and hg.pr_trace.size < hg.T and (np.diff(hg.pr_trace) < 0).any(), name
        assert (hg.pr_len != hg.len_t[hg.pr_trace]).any(), name
    if fused:
        assert hg.rs_off is None and hg.N <= FX_NMAX
        return
    assert hg.rs_ops.size != hg.sr_ops.size or not np.array_equal(hg.rs_ops, hg.sr_ops)
    if name == "one_trace":
        assert (hg.T, r.n_tiles) == (1, 1)
    elif name == "ragged_tile":
        assert r.n_tiles == 1 and hg.T % 256
    elif name == "six_tiles":
        assert r.n_tiles == 6 and hg.T % 256 == 0
    elif name == "long_pairs":
        assert r.n_tiles == 6 and hg.T % 256 and r.long_pairs >= 1 and r.max_block_ids > VCAP
    elif name == "su_global":
        assert hg.N > LDS_NODES and r.max_row > VCAP and r.long_pairs >= 1 and r.max_block_ids > 2 * VCAP
    elif name == "int32_ids":
        assert hg.N > U16_NODES and r.n_tiles == 6
    elif name == "tshift9":
        assert (hg.T >> 8) > 256 and r.tshift == 9 and r.n_tiles == -(-hg.T // 512) and r.long_pairs >= 1
    if hg.T >= 200:   # empty traces and list multiplicities are in
        assert (hg.len_t == 0).any() and (hg.len_t > np.diff(hg.sr_off)).any()
        assert (hg.len_o > np.bincount(hg.rs_ops, minlength=hg.N)).any()
        assert (hg.nchild > np.bincount(hg.ss_par, minlength=hg.N)).any()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's graph, its host arrays and the oracle's results (computed once, read-only)."""
    N, T, knobs = CASES[name]
    g = general_graph(N, T, SEED, **knobs)
    return _with_oracle(g, host_graph_from_oracle(g))


def _with_oracle(g, hg):
    kind = orc.trace_kinds(g)
    ref = {}
    for anomaly in (False, True):
        v = orc.preference(g, kind, anomaly)
        w, cov = orc.weights(g, orc.power_iteration(g, v))
        ref[anomaly] = (v, np.array(list(w.values())), np.array(list(cov.values())))
    shared = [kind, *ref[False], *ref[True]] + [x for x in vars(hg).values() if isinstance(x, np.ndarray)]
    for a in shared:   # shared among the tests: nobody writes
        a.setflags(write=False)
    return types.SimpleNamespace(g=g, hg=hg, kind=kind, ref=ref)


def _upload(hg):
    from microrank_amd import _lib
    from microrank_amd.graph import DeviceGraph

    return DeviceGraph.upload(_lib.default_context(), hg)


def _assert_fp64(w, w_ref, what):
    err = np.abs(w - w_ref)[w_ref > 0] / w_ref[w_ref > 0]
    print(f"{what}: fp64 max rel diff vs oracle {err.max() if err.size else 0.0:.3e}, "
          f"zeros {int((w_ref == 0).sum())}, smallest nonzero {w_ref[w_ref > 0].min():.3e}")
    assert ((w == 0) == (w_ref == 0)).all(), what
    np.testing.assert_allclose(w, w_ref, rtol=RTOL64, atol=0, err_msg=what)


def _assert_fp32(w, w_ref, masked, what):
    m = w_ref >= 1e-6 * w_ref.max() if masked else np.ones(w_ref.size, bool)   # test_c4_full_scale_properties' rule
    err = np.abs(w[m] - w_ref[m])[w_ref[m] > 0] / w_ref[m][w_ref[m] > 0]
    print(f"{what}: fp32 max rel diff vs oracle {err.max():.3e} over {int(m.sum())} of {m.size} ops")
    np.testing.assert_allclose(w[m], w_ref[m], rtol=RTOL32, atol=0, err_msg=what)


PARITY_CASES = [n for n in CASES if n != "su_global_rs_is_sr"]


@pytest.mark.parametrize("anomaly", [False, True])
@pytest.mark.parametrize("name", PARITY_CASES)
def test_general_graph_against_oracle(name, anomaly):
    c = _case(name)
    _assert_regime(name, c.hg)
    v, w_ref, cov_ref = c.ref[anomaly]
    dg = _upload(c.hg)
    # reference-order preference sums: the oracle's preference bit for bit
    dg.pagerank(anomaly, exact_sums=True)
    w, cov, kind, pref = dg.fetch(kinds=True)
    np.testing.assert_array_equal(kind, c.kind)
    assert pref.tobytes() == v.tobytes(), "preference with exact sums is not the oracle's, bit for bit"
    np.testing.assert_array_equal(cov, cov_ref)
    _assert_fp64(w, w_ref, f"{name} anomaly={anomaly} exact_sums")
    # default flags: tree sums
    dg.pagerank(anomaly)
    w, cov, kind, pref = dg.fetch(kinds=True)
    np.testing.assert_array_equal(kind, c.kind)
    assert ((pref == 0) == (v == 0)).all()
    np.testing.assert_allclose(pref, v, rtol=PREF_ULP, atol=0)
    np.testing.assert_array_equal(cov, cov_ref)
    _assert_fp64(w, w_ref, f"{name} anomaly={anomaly}")
    dg.pagerank(anomaly)
    w2, cov2, kind2, pref2 = dg.fetch(kinds=True)
    assert (w2.tobytes(), cov2.tobytes(), kind2.tobytes(), pref2.tobytes()) == \
        (w.tobytes(), cov.tobytes(), kind.tobytes(), pref.tobytes()), "rerun not bitwise identical"
    if name in FP32_FULL + FP32_MASKED:
        dg.pagerank(anomaly, precision="fp32")
        w3, cov3 = dg.fetch()
        np.testing.assert_array_equal(cov3, cov_ref)
        _assert_fp32(w3, w_ref, name in FP32_MASKED, f"{name} anomaly={anomaly}")
        dg.pagerank(anomaly, precision="fp32")
        assert dg.fetch()[0].tobytes() == w3.tobytes(), "fp32 rerun not bitwise identical"
    dg.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("anomaly", [False, True])
def test_general_dicts_against_reference(anomaly, precision):
    """The recorded general dicts through trace_pagerank (the product's own dict conversion) against
    the reference's output on them: key orders and counts exact, weights 1e-10 / 1e-4."""
    from microrank_amd.graph import host_graph_from_dicts
    from microrank_amd.pagerank import trace_pagerank

    fix = load_golden("dict_general.json")
    dicts = general_golden_dicts(fix)
    _assert_regime("long_pairs", host_graph_from_dicts(*dicts))
    exp = fix[f"anomaly={anomaly}"]
    w, num = trace_pagerank(*dicts, anomaly, precision=precision)
    assert list(w.keys()) == exp["keys"] and list(num.keys()) == exp["num_keys"]
    assert [int(x) for x in num.values()] == exp["num"]
    assert all(isinstance(x, np.float64) for x in w.values())
    got, ref = np.array(list(w.values())), unhex(exp["weight"])
    if precision == "fp64":
        _assert_fp64(got, ref, f"reference anomaly={anomaly}")
    else:
        _assert_fp32(got, ref, False, f"reference anomaly={anomaly}")


def _forced_tiles(hg):
    """The same graph with P_rs given explicitly (copies of the sr arrays): never fused."""
    assert hg.rs_off is None
    return dataclasses.replace(hg, rs_off=hg.sr_off.copy(), rs_ops=hg.sr_ops.copy())


@pytest.mark.parametrize("anomaly", [False, True])
@pytest.mark.parametrize("name", ["fused_pr_subset", "su_global_rs_is_sr"])
def test_forced_tile_path_against_fused(name, anomaly):
    """One rs == sr graph on both iterations: uploaded as it is (fused) and with explicit rs arrays
    equal to the sr arrays (tiles).  Both within 1e-10 of the oracle, hence of each other; kinds,
    preference and coverage identical.  The two sum in different orders, so the weights need not be
    byte-equal (printed)."""
    c = _case(name)
    _assert_regime(name, c.hg)
    tiles = _forced_tiles(c.hg)
    r = _regime(tiles)
    assert r.tile_path and r.long_pairs >= 1 and r.max_block_ids > VCAP
    if name == "su_global_rs_is_sr":
        assert tiles.N > LDS_NODES and r.max_row > VCAP
    v, w_ref, cov_ref = c.ref[anomaly]
    out = []
    for form, hg in (("fused", c.hg), ("tiles", tiles)):
        dg = _upload(hg)
        dg.pagerank(anomaly)
        w, cov, kind, pref = dg.fetch(kinds=True)
        np.testing.assert_array_equal(kind, c.kind)
        np.testing.assert_array_equal(cov, cov_ref)
        np.testing.assert_allclose(pref, v, rtol=PREF_ULP, atol=0)
        _assert_fp64(w, w_ref, f"{name} {form} anomaly={anomaly}")
        out.append((w, cov, kind, pref))
        dg.close()
    (w_f, cov_f, k_f, p_f), (w_t, cov_t, k_t, p_t) = out
    assert (cov_f.tobytes(), k_f.tobytes(), p_f.tobytes()) == (cov_t.tobytes(), k_t.tobytes(), p_t.tobytes())
    print(f"{name} anomaly={anomaly}: fused vs tile weights byte-equal: {w_f.tobytes() == w_t.tobytes()}, "
          f"max rel diff {np.max(np.abs(w_f - w_t)[w_t > 0] / w_t[w_t > 0]):.3e}")


@pytest.mark.parametrize("name", ["long_pairs", "su_global", "int32_ids"])
def test_kinds_by_partition_on_general_graphs(name, monkeypatch):
    """The partition form of the kinds (forced with MR_KIND_PART_MIN=0, read per call) on graphs whose
    kind keys come from int32 ids of the sr arrays (k_kind_rec<4>, k_kind_final<int32_t>): the
    oracle's kinds exactly, and the hash-table run's weights byte for byte."""
    c = _case(name)
    dg = _upload(c.hg)
    monkeypatch.setenv("MR_KIND_PART_MIN", "1000000000")
    dg.pagerank(True)
    w0, _, k0, p0 = dg.fetch(kinds=True)
    monkeypatch.setenv("MR_KIND_PART_MIN", "0")
    dg.pagerank(True)
    w1, _, k1, p1 = dg.fetch(kinds=True)
    np.testing.assert_array_equal(k0, c.kind)
    np.testing.assert_array_equal(k1, c.kind)
    assert p1.tobytes() == p0.tobytes() and w1.tobytes() == w0.tobytes()
    dg.close()


@pytest.mark.parametrize("name", ["long_pairs", "fused_pr_subset"])
def test_kind_compress_falls_back_off_its_surface(name):
    """compress_kinds on a graph off the fused path, and on a fused graph whose pr_trace is not
    operation_trace, ranks uncompressed (kind_compressed_pagerank): the plain call's bytes."""
    c = _case(name)
    dg = _upload(c.hg)
    for anomaly in (False, True):
        dg.pagerank(anomaly)
        plain = dg.fetch(kinds=True)
        dg.pagerank(anomaly, compress_kinds=True)
        comp = dg.fetch(kinds=True)
        assert [a.tobytes() for a in comp] == [a.tobytes() for a in plain]
        _assert_fp64(comp[0], c.ref[anomaly][1], f"{name} compress_kinds anomaly={anomaly}")
    dg.close()


@functools.lru_cache(maxsize=None)
def _span_case():
    """A graph as get_pagerank_graph builds it (fused, batched set-up): 40 ops, 300 traces."""
    from microrank_amd import synth

    st = synth.gen_spans(synth.make_topology(40, 3), 300, 4, branch=4.0, p_max=0.7, names=False)
    g = orc.span_graph(st.trace, st.podop, st.span, st.parent, np.ones(st.n_traces, dtype=bool)).as_graph()
    hg = host_graph_from_oracle(g)
    assert hg.rs_off is None and hg.pr_trace is None
    return _with_oracle(g, hg)


BATCH = ("span", "long_pairs", "fused_pr_subset", "su_global")
BATCH_ANOMALY = (0, 1, 1, 0)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_mixed_batch_of_fused_and_tile_graphs(precision, reverse):
    """One mr_pagerank_batch call over fused and tile-path graphs: k_iter_a's and k_iter_b's block
    -> graph search runs over graphs that have no block in the launch, next to the fused launches'.
    Each graph: kinds and preference byte-equal to its own ranking's, weights within 1e-12 of it
    (test_gpu_setup_paths' bound for batched against alone) and within the oracle tolerances."""
    from microrank_amd import _lib

    names, anomaly = list(BATCH), list(BATCH_ANOMALY)
    if reverse:
        names.reverse()
        anomaly.reverse()
    cases = [_span_case() if n == "span" else _case(n) for n in names]
    fused = [not _regime(c.hg).tile_path for c in cases]
    assert sorted(fused) == [False, False, True, True]
    ctx = _lib.default_context()
    lib = _lib.load()
    dgs = [_upload(c.hg) for c in cases]
    alone = []
    for dg, a in zip(dgs, anomaly):
        dg.pagerank(bool(a), precision=precision)
        alone.append(dg.fetch(kinds=True))
    hs = (_lib.P * len(dgs))(*[dg.h for dg in dgs])
    an = (C.c_int * len(dgs))(*anomaly)
    prec = _lib.MR_FP32 if precision == "fp32" else _lib.MR_FP64
    ctx.check(lib.mr_pagerank_batch(ctx.h, hs, an, len(dgs), 0.85, 0.01, 25, prec, 0), "mr_pagerank_batch")
    for n, c, a, dg, (w_a, cov_a, k_a, p_a) in zip(names, cases, anomaly, dgs, alone):
        w, cov, k, p = dg.fetch(kinds=True)
        v, w_ref, cov_ref = c.ref[bool(a)]
        what = f"batch {n} {precision} reverse={reverse}"
        np.testing.assert_array_equal(k, c.kind, err_msg=what)
        assert (k.tobytes(), p.tobytes(), cov.tobytes()) == (k_a.tobytes(), p_a.tobytes(), cov_a.tobytes()), what
        np.testing.assert_array_equal(cov, cov_ref, err_msg=what)
        np.testing.assert_allclose(p, v, rtol=PREF_ULP, atol=0, err_msg=what)
        print(f"{what}: weights batched vs alone byte-equal: {w.tobytes() == w_a.tobytes()}, max rel diff "
              f"{np.max(np.abs(w - w_a)[w_a > 0] / w_a[w_a > 0]):.3e}")
        np.testing.assert_allclose(w, w_a, rtol=1e-12, atol=0, err_msg=what)
        if precision == "fp64":
            _assert_fp64(w, w_ref, what)
        elif n in FP32_FULL + FP32_MASKED:
            _assert_fp32(w, w_ref, n in FP32_MASKED, what)
    for dg in dgs:
        dg.close()


def _descriptor(hg):
    """The mr_graph_desc DeviceGraph.upload passes, pointing into copies of the arrays (returned)."""
    from microrank_amd._lib import GraphDesc, ptr

    a = {f: np.array(getattr(hg, f), order="C") for f in ("sr_off", "sr_ops", "rs_off", "rs_ops", "len_t", "len_o",
                                                            "ss_off", "ss_par", "nchild", "pr_trace", "pr_len")}
    d = GraphDesc()
    d.n_nodes, d.n_traces = hg.N, hg.T
    d.nnz_sr, d.nnz_rs, d.n_edges, d.n_pr = a["sr_ops"].size, a["rs_ops"].size, a["ss_par"].size, a["pr_trace"].size
    for f, ct in (("sr_off", C.c_int64), ("sr_ops", C.c_int32), ("rs_off", C.c_int64), ("rs_ops", C.c_int32),
                  ("len_t", C.c_int32), ("len_o", C.c_int32), ("ss_off", C.c_int64), ("ss_par", C.c_int32),
                  ("nchild", C.c_int32), ("pr_trace", C.c_int32), ("pr_len", C.c_int32)):
        setattr(d, f, ptr(a[f], ct))
    return d, a


def _rs_op_too_large(d, a, hg):
    a["rs_ops"][a["rs_ops"].size // 2] = hg.N


def _rs_op_negative(d, a, hg):
    a["rs_ops"][0] = -1


def _rs_off_end(d, a, hg):
    a["rs_off"][hg.T] += 1


def _rs_off_without_ops(d, a, hg):
    d.rs_ops = C.cast(None, C.POINTER(C.c_int32))


def _pr_trace_too_large(d, a, hg):
    a["pr_trace"][a["pr_trace"].size // 2] = hg.T


def _pr_trace_negative(d, a, hg):
    a["pr_trace"][0] = -1


def _sr_off_start(d, a, hg):
    a["sr_off"][0] = 1


@pytest.mark.parametrize("spoil", [_rs_op_too_large, _rs_op_negative, _rs_off_end, _rs_off_without_ops,
                                   _pr_trace_too_large, _pr_trace_negative, _sr_off_start],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_upload_rejects_malformed_general_descriptors(spoil):
    """Descriptors mr_graph_upload's host checks reject (before any kernel reads them): MR_ERR_ARG, no
    handle, and the context ranks a good graph afterwards."""
    from microrank_amd import _lib

    c = _case("long_pairs")
    ctx = _lib.default_context()
    lib = _lib.load()
    d, a = _descriptor(c.hg)
    h = _lib.P()
    assert lib.mr_graph_upload(ctx.h, C.byref(d), C.byref(h)) == _lib.MR_OK and h.value   # the unspoilt one is good
    assert lib.mr_graph_free(h) == _lib.MR_OK
    spoil(d, a, c.hg)
    h = _lib.P()
    assert lib.mr_graph_upload(ctx.h, C.byref(d), C.byref(h)) == _lib.MR_ERR_ARG
    assert not h.value
    dg = _upload(c.hg)
    dg.pagerank(True)
    w, cov, kind, _ = dg.fetch(kinds=True)
    np.testing.assert_array_equal(kind, c.kind)
    np.testing.assert_array_equal(cov, c.ref[True][2])
    _assert_fp64(w, c.ref[True][1], "after a rejected upload")
    dg.close()
