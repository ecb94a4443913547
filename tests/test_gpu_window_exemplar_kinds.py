"""One exemplar per trace kind for a window batch on the GPU: mr_windows_batch_exemplars_ex with
MR_EX_DISTINCT_KINDS through rank_windows(..., exemplars=m, exemplar_kinds=True), and the driver's
5-column exemplars.csv.

Windows and their oracle side: window_exemplar_cases (unchanged); the kinds of a window are
exemplar_kinds_util.kind_ids of its graph of the detector's abnormal traces.  `ties` is the case whose
op rows hold fewer than 32 kinds for some ops and more for others.

Bounds: a returned score against the oracle's r_K 1e-9 relative (fp64, 25 iterations).  Kind identity
is claimed where the oracle separates a representative from both neighbours by more than that; counts
(ex_n) and class sizes (ex_mult) are exact everywhere.  Between the layout-order build and the general
build scores agree to 1e-9, kinds and class sizes wherever the oracle separates neighbours by more
than 1e-8 (test_gpu_window_exemplars' route bounds: the builds order their sums differently).
"""
import contextlib
import csv
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import window_exemplar_cases as wc
from conftest import load_golden
from exemplar_kinds_util import distinct_top, kind_ids

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ROUTE_SEP = 1e-8
MS = (8, 32)
K = wc.ITERS["fp64"]
KNOBS = ("MR_EX_BLOCKS", "MR_WIN_GROUP", "MR_WIN_CHUNK", "MR_TR_MERGE", "MR_NO_LO", "MR_NO_LO_WIN", "MR_NO_INDEX",
         "MR_KIND_TEST_COLLIDE")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def ctx():
    from microrank_amd import _lib

    return _lib.default_context()


@pytest.fixture(scope="module")
def wins(ctx):
    """name -> (DeviceSpans, t0, t1, a3, ok)."""
    from microrank_amd.anormaly_detector import slo_arrays
    from microrank_amd.preprocess_data import DeviceSpans

    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        devs = {n: DeviceSpans(ctx, wc.table(n)[0]) for n in wc.NAMES}
    out = {}
    for n in wc.NAMES:
        st, slo, _, t0, t1 = wc.table(n)
        a3, ok = slo_arrays(st, slo)
        out[n] = (devs[n], t0, t1, a3, ok)
    yield out
    for d in devs.values():
        d.close()


@functools.lru_cache(maxsize=None)
def kinds(name):
    """(kid, class size) by trace index of the window's graph of abnormal traces."""
    g = wc.graphs(name)[0][0]
    kid = kind_ids(g)
    size = np.bincount(kid)[kid]
    kid.setflags(write=False)
    size.setflags(write=False)
    return kid, size


def _rank(ctx, ws, m, kinds_=True, **kw):
    from microrank_amd.online_rca import rank_windows

    kw.setdefault("iters", K)
    return rank_windows(ctx, ws, exemplars=m, exemplar_kinds=kinds_, **kw)


def _bits(res):
    six = (res[0].tobytes(), res[1].tobytes()) + tuple(res[2:6])
    return six + (tuple((c, tuple((r[0], r[1].tobytes()) + tuple(r[2:]) for r in lst)) for c, lst in res[6].items()),)


def _check(name, res, m, plain=None):
    """One window's answer against the oracle."""
    from microrank_amd import _lib

    o = wc.oracle(name, K)
    kid, size = kinds(name)
    assert len(res) == 7 and res[5] == _lib.MR_OK and (res[2], res[3]) == (o.n_abnormal, o.n_normal)
    codes, ex = res[0].tolist(), res[6]
    assert codes == o.top and list(ex) == codes
    worst, fewer, more = 0.0, 0, 0
    for code in codes:
        lst, what = ex[code], f"{name} m={m} pod-op {code}"
        row = o.rows.get(code)
        if row is None:
            assert lst == [], what
            continue
        reps = distinct_top(row, o.r, kid, len(row))   # every kind of the row, in the oracle's order
        n = min(m, reps.size)
        fewer += reps.size < m
        more += reps.size > m
        assert len(lst) == n, f"{what}: {len(lst)} entries, {reps.size} kinds"
        assert all(len(x) == 3 and isinstance(x[1], np.float64) and isinstance(x[2], int) for x in lst), what
        tr = np.array([x[0] for x in lst], np.int64)
        sc = np.array([x[1] for x in lst], np.float64)
        mu = np.array([x[2] for x in lst], np.int64)
        gi = np.minimum(np.searchsorted(o.trace_codes, tr), o.trace_codes.size - 1)
        assert (o.trace_codes[gi] == tr).all() and np.isin(gi, row).all(), what
        assert len(set(kid[gi].tolist())) == n, f"{what}: a kind twice"
        np.testing.assert_array_equal(mu, size[gi], err_msg=what)        # exact, whichever member stands for the kind
        assert (np.diff(sc) <= 0).all(), what
        same = np.flatnonzero(sc[1:].view(np.uint64) == sc[:-1].view(np.uint64))
        assert (tr[same + 1] > tr[same]).all(), f"{what}: equal scores not in trace code order"
        s = o.r[reps]
        np.testing.assert_allclose(sc, s[:n], rtol=RTOL, atol=0, err_msg=what)
        np.testing.assert_allclose(sc, o.r[gi], rtol=RTOL, atol=0, err_msg=what)
        worst = max(worst, float(np.max(np.abs(sc - s[:n]) / s[:n])))
        gap = s[:-1] - s[1:]
        apart = np.minimum(np.concatenate(([np.inf], gap)), np.concatenate((gap, [np.inf])))[:n] > RTOL * s[:n]
        np.testing.assert_array_equal(kid[gi][apart], kid[reps[:n]][apart], err_msg=what)
        # every listed trace is its kind's best member up to the bound
        for g_, k_ in zip(gi, kid[gi]):
            mem = row[kid[row] == k_]
            assert o.r[g_] >= o.r[mem].max() * (1 - RTOL), what
        if plain is not None and n:
            assert (lst[0][0], lst[0][1].tobytes()) == (plain[6][code][0][0], plain[6][code][0][1].tobytes()), what
    print(f"{name} m={m}: max rel diff vs the oracle's representatives {worst:.3e}; rows with fewer kinds than m {fewer}, more {more}")
    return fewer, more


# ---------------------------------------------------------------------------- 1. / 4. against the oracle
@pytest.mark.parametrize("m", MS)
def test_against_oracle(ctx, wins, m):
    every = [wins[n] for n in wc.NAMES]
    plain = _rank(ctx, every, m, False)
    batch = _rank(ctx, every, m)
    seen = {}
    for n, res, p in zip(wc.NAMES, batch, plain):
        assert _bits(res)[:6] == _bits(p)[:6], f"{n}: the keyword changed the ranking"
        seen[n] = _check(n, res, m, p)
    if m == 32:   # `ties`: rows below and above the cut
        assert seen["ties"][1] >= 1
    for n in wc.NAMES:
        (alone,) = _rank(ctx, [wins[n]], m)
        assert _bits(alone) == _bits(batch[wc.NAMES.index(n)]), n
    assert any(lst == [] for lst in batch[wc.NAMES.index("one_trace")][6].values())


def _raw(ctx, ws, m, flags, mult=True, fill=7, ex=True, top_max=5):
    """mr_windows_batch_exemplars_ex (ex=False: mr_windows_batch_exemplars) itself, outputs pre-filled."""
    from microrank_amd import _lib
    from microrank_amd._lib import ptr

    n, k = len(ws), top_max + 6
    spans = (_lib.P * n)(*[w[0].h for w in ws])
    t0, t1 = np.array([w[1] for w in ws], np.int64), np.array([w[2] for w in ws], np.int64)
    a3 = (C.c_void_p * n)(*[w[3].ctypes.data for w in ws])
    ok = (C.c_void_p * n)(*[w[4].ctypes.data for w in ws])
    codes, scores = np.zeros(n * k, np.int32), np.zeros(n * k)
    n_out, na, nn, status = (np.zeros(n, np.int32) for _ in range(4))
    edges = np.zeros(n, np.int64)
    nm = n * k * max(m, 1)
    ex_t, ex_s, ex_c = np.full(nm, fill, np.int32), np.full(nm, float(fill)), np.full(n * k, fill, np.int32)
    ex_m = np.full(nm, fill, np.int32)
    args = (ctx.h, n, spans, ptr(t0, C.c_int64), ptr(t1, C.c_int64), a3, ok, 0, top_max, _lib.MR_FP64,
            ptr(codes, C.c_int32), ptr(scores, C.c_double), ptr(n_out, C.c_int32), ptr(edges, C.c_int64),
            ptr(na, C.c_int32), ptr(nn, C.c_int32), ptr(status, C.c_int32), K, 0.0, 1, None, None, m,
            ptr(ex_t, C.c_int32), ptr(ex_s, C.c_double), ptr(ex_c, C.c_int32))
    lib = _lib.load()
    rc = lib.mr_windows_batch_exemplars_ex(*args, flags, ptr(ex_m, C.c_int32) if mult else None) if ex else \
        lib.mr_windows_batch_exemplars(*args)
    return rc, n_out, ex_t.reshape(n, k, -1), ex_s.reshape(n, k, -1), ex_c.reshape(n, k), ex_m.reshape(n, k, -1), status


def test_padding_arguments_and_the_plain_call(ctx, wins):
    from microrank_amd import _lib

    DK = _lib.MR_EX_DISTINCT_KINDS
    dev, t0, t1, a3, ok = wins["one_trace"]
    ws = [wins["ties"], wins["one_trace"],
          (dev, t0, t1, a3 * 1e6, ok),                     # no abnormal trace: nothing ranked
          (dev, t1 + 10**12, t1 + 2 * 10**12, a3, ok)]     # an empty window
    rc, n_out, tr, sc, cnt, mu, status = _raw(ctx, ws, 32, DK)
    assert rc == _lib.MR_OK and n_out.tolist()[:2] == [wc.K_TOP] * 2 and n_out.tolist()[2:] == [0, 0]
    assert status.tolist() == [_lib.MR_OK, _lib.MR_OK, _lib.MR_OK, _lib.MR_ERR_VALUE]
    for i, name in enumerate(("ties", "one_trace")):
        o = wc.oracle(name, K)
        kid, size = kinds(name)
        want = [min(32, np.unique(kid[o.rows[c]]).size) if c in o.rows else 0 for c in o.top]
        assert cnt[i].tolist() == want, name
        for j, c in enumerate(cnt[i]):
            assert (tr[i, j, :c] >= 0).all() and (sc[i, j, :c] > 0).all() and (mu[i, j, :c] >= 1).all()
            assert (tr[i, j, c:] == -1).all() and (sc[i, j, c:] == 0.0).all() and (mu[i, j, c:] == 0).all()
    assert (cnt[0] == 32).any()
    assert (cnt[1] == 0).any()   # an op only normal traces hold
    for i in (2, 3):             # windows that ranked nothing
        assert (tr[i] == -1).all() and (sc[i] == 0.0).all() and (cnt[i] == 0).all() and (mu[i] == 0).all()
    ws = ws[:2]
    assert _raw(ctx, ws, 8, DK, mult=False)[0] == _lib.MR_OK          # ex_mult may be NULL
    for flags in (2, 3, 0x80000000):
        assert _raw(ctx, ws, 8, flags)[0] == _lib.MR_ERR_ARG, flags
    assert _raw(ctx, ws, 8, 0)[0] == _lib.MR_ERR_ARG                  # ex_flags == 0 with ex_mult
    for m in (0, 33, -1):
        assert _raw(ctx, ws, m, DK)[0] == _lib.MR_ERR_ARG, m
    assert _raw(ctx, ws, 4, DK, top_max=59)[0] == _lib.MR_ERR_ARG
    # ex_flags == 0, NULL is mr_windows_batch_exemplars, bit for bit
    a = _raw(ctx, ws, 32, 0, mult=False)
    b = _raw(ctx, ws, 32, 0, ex=False)
    assert a[0] == b[0] == _lib.MR_OK
    assert [x.tobytes() for x in a[1:5]] == [x.tobytes() for x in b[1:5]]
    assert (a[5] == 7).all()   # (never written)


# ---------------------------------------------------------------------------- 2. cuts, grouping, place
@pytest.mark.parametrize("knob,values", [("MR_EX_BLOCKS", ("1", "3")), ("MR_WIN_GROUP", ("1",)), ("MR_WIN_CHUNK", ("1",))])
def test_cuts_do_not_change_the_answer(ctx, wins, monkeypatch, knob, values):
    every = [wins[n] for n in wc.NAMES]
    for m in MS:
        want = [_bits(r) for r in _rank(ctx, every, m)]
        assert any(r[6] for r in want)
        for v in values:
            monkeypatch.setenv(knob, v)
            assert [_bits(r) for r in _rank(ctx, every, m)] == want, (knob, v, m)
        monkeypatch.delenv(knob)


@pytest.mark.parametrize("name", wc.NAMES)
def test_position_in_the_call(ctx, wins, name):
    (alone,) = _rank(ctx, [wins[name]], 32)
    others = [wins[n] for n in wc.NAMES if n != name][:3]
    five = _rank(ctx, [wins[name]] + others + [wins[name]], 32)
    assert _bits(five[0]) == _bits(alone) == _bits(five[4]), name


def test_stop_at_tol(ctx, wins):
    every = [wins[n] for n in wc.NAMES]
    info = []
    got = _rank(ctx, every, 8, tol=1e-6, iters=60, check_every=4, info=info)
    for k in sorted({i["iters"] for i in info}):
        assert 1 <= k < 60
        fixed = _rank(ctx, every, 8, iters=k)
        for n, i, a, b in zip(wc.NAMES, info, got, fixed):
            if i["iters"] == k:
                assert _bits(a) == _bits(b), n
    assert any(r[6] and any(r[6].values()) for r in got)


def test_run_merged_graphs(ctx, wins, monkeypatch):
    got = {}
    for v in ("1", "2"):
        monkeypatch.setenv("MR_TR_MERGE", v)
        (got[v],) = _rank(ctx, [wins["ties"]], 32)
        _check("ties", got[v], 32)
    assert _bits(got["1"]) == _bits(got["2"])


# ---------------------------------------------------------------------------- 3. routes
@pytest.mark.parametrize("name", ["ragged", "mid", "ties"])
def test_routes_agree(ctx, wins, monkeypatch, name):
    o = wc.oracle(name, K)
    kid, _ = kinds(name)
    for m in MS:
        monkeypatch.delenv("MR_NO_LO_WIN", raising=False)
        (base,) = _rank(ctx, [wins[name]], m)
        monkeypatch.setenv("MR_NO_LO_WIN", "1")   # the batch's general build: through mr_graph_exemplars_ex
        (gen,) = _rank(ctx, [wins[name]], m)
        _check(name, gen, m)
        assert base[0].tolist() == gen[0].tolist() and base[2:6] == gen[2:6]
        for code in base[0].tolist():
            la, lb = base[6][code], gen[6][code]
            assert len(la) == len(lb), (name, code)   # ex_n
            if not la:
                continue
            np.testing.assert_allclose([x[1] for x in lb], [x[1] for x in la], rtol=RTOL, atol=0, err_msg=f"{name} {code}")
            row = o.rows[code]
            reps = distinct_top(row, o.r, kid, len(row))
            s = o.r[reps]
            gap = s[:-1] - s[1:]
            apart = np.minimum(np.concatenate(([np.inf], gap)), np.concatenate((gap, [np.inf])))[:len(la)] > ROUTE_SEP * s[:len(la)]
            ga = np.searchsorted(o.trace_codes, [x[0] for x in la])
            gb = np.searchsorted(o.trace_codes, [x[0] for x in lb])
            np.testing.assert_array_equal(kid[ga][apart], kid[gb][apart], err_msg=f"{name} {code}: kinds")
            np.testing.assert_array_equal(np.array([x[2] for x in la])[apart], np.array([x[2] for x in lb])[apart])


# ---------------------------------------------------------------------------- 6. Python and the driver
def test_rank_windows_returns_triples(ctx, wins):
    every = [wins[n] for n in wc.NAMES]
    old = _rank(ctx, every, 8, False)
    new = _rank(ctx, every, 8)
    for a, b in zip(old, new):
        assert list(a[6]) == list(b[6])
        assert all(len(x) == 2 for lst in a[6].values() for x in lst)
        assert all(len(x) == 3 for lst in b[6].values() for x in lst)


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
    return buf.getvalue(), err


def test_driver_writes_the_traces_column(ctx, tmp_path, monkeypatch):
    from microrank_amd import synth

    case = load_golden("stream.json")
    _, adf = synth.stream_dataframes(**case["params"])
    monkeypatch.chdir(tmp_path)
    out3 = _driver(adf, case, exemplars=3)
    res3, ex3 = open("result.csv", "rb").read(), open("exemplars.csv", "rb").read()
    assert list(csv.DictReader(io.StringIO(ex3.decode())).fieldnames) == ["result", "rank", "trace", "score"]
    os.remove("exemplars.csv")
    outk = _driver(adf, case, exemplars=3, exemplar_kinds=True)
    assert outk == out3 and open("result.csv", "rb").read() == res3
    rows = list(csv.DictReader(open("exemplars.csv")))
    assert rows and list(rows[0]) == ["result", "rank", "trace", "score", "traces"]
    old = list(csv.DictReader(io.StringIO(ex3.decode())))
    first = {r["result"]: r for r in reversed(old) if r["rank"] == "1"}
    per = {}
    for r in rows:
        per.setdefault(r["result"], []).append(r)
    for op, rs in per.items():
        assert len(rs) <= 3 and [int(r["rank"]) for r in rs] == list(range(1, len(rs) + 1))
        sc = [float(r["score"]) for r in rs]
        assert sc == sorted(sc, reverse=True) and all(int(r["traces"]) >= 1 for r in rs)
        assert (rs[0]["trace"], rs[0]["score"]) == (first[op]["trace"], first[op]["score"])   # entry 0 is the plain one
    # without the keyword the file is what the old keyword set writes
    os.remove("exemplars.csv")
    assert _driver(adf, case, exemplars=3, exemplar_kinds=False) == out3
    assert open("exemplars.csv", "rb").read() == ex3
