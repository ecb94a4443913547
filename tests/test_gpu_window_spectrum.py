"""The window routes of the spectrum step -- k_win_spectrum / k_win_spectrum_b (union, scores, sort
and top k in one block) and the general route (k_union_* + mr_spectrum_dev) -- for all 13
formulas, on windows whose two graphs each have nodes the other lacks, and at the limits of the
one-block route.

The suite's other windows come from bench.make_window as it is: the graph ranked as anomaly_result
(the detector's large normal list, T1) then covers every op the other graph has, so no window has
a normal-only node.  Here every odd-numbered trace is made slow, which splits the window about in
half.  Measured with the numpy oracle (SLO, detector, two span graphs):

    seed, ops, traces    Na    Nn  anomaly-only  normal-only  union  pod-ops  route
    21,  600,  800      566   575       20           29         595     600   one block
    26, 2100, 3500     2024  1986       83           45        2069    2100   one block (m = 4096, two
                                                                              normal nodes per thread)
    22, 2500, 3000     2237  2232      139          134        2371    2500   general (Na + Nn = 4469)
    24, 5200, 6000     3762  3782      580          600        4362    5200   general (NP > 4096; the
                                                                              union's 4362 keys: radix sort)

Each window's counts and route are asserted on the oracle's graphs (``window`` below), so a drift
of the generator fails loudly instead of testing nothing.  The two tests without the gpu mark
check the windows and the oracle's own rank separation on the CPU."""
import functools

import numpy as np
import pytest

import oracle as orc

WINDOWS = {"small": (21, 600, 800), "mid": (26, 2100, 3500), "over": (22, 2500, 3000), "big": (24, 5200, 6000)}
# (Na, Nn, anomaly-only, normal-only, pod-ops) as measured; the route follows from them
MEASURED = {"small": (566, 575, 20, 29, 600), "mid": (2024, 1986, 83, 45, 2100), "over": (2237, 2232, 139, 134, 2500),
            "big": (3762, 3782, 580, 600, 5200)}
WS_MAX, WS_PMAX, WS_KMAX, WS_T = 4096, 4096, 256, 1024   # mr_spectrum.hip
K = 256                                                 # top_max = 250
METHODS = orc.SPECTRUM_METHODS


def fits(Na, Nn, NP, k):
    """mr_win_spectrum_fits."""
    return Na + Nn <= WS_MAX and NP <= WS_PMAX and 0 <= k <= WS_KMAX


class Window:
    pass


@functools.lru_cache(maxsize=None)
def window(name):
    """The window's tables, SLO and the oracle's side of it (online_rca.py:164-201 up to the two
    PageRanks; the spectrum per method in ``oracle_spectrum``), with the preconditions of the tests."""
    import bench

    seed, ops, traces = WINDOWS[name]
    w = Window()
    _, normal, ab = bench.make_window(seed, ops, traces)
    ab.duration = np.where(ab.trace % 2 == 1, ab.duration * 1000, ab.duration)   # every odd trace is slow
    w.table, w.t0 = ab, int(ab.tstart.min())
    w.t1 = w.t0 + 5 * 60 * 10**9
    assert ab.svcop_names == normal.svcop_names
    w.slo = orc.operation_slo(normal.svcop, normal.duration, normal.svcop_names, normal.svcop_names)
    w.a3, w.ok = np.zeros(ab.n_svcops), np.zeros(ab.n_svcops, np.uint8)
    for code, nm in enumerate(ab.svcop_names):
        if nm in w.slo:
            w.a3[code], w.ok[code] = w.slo[nm][0] + 3 * w.slo[nm][1], 1
    a3map = {i: float(w.a3[i]) for i in range(len(w.a3)) if w.ok[i]}
    _, abn, nor = orc.detect(ab.trace, ab.svcop, ab.duration, ab.tstart, ab.tend, w.t0, w.t1, a3map)
    w.n_abnormal, w.n_normal = len(abn), len(nor)
    w.pr = {}
    for lst, anomaly in ((abn, False), (nor, True)):   # normal_list = the detector's abnormal traces (T1)
        sel = np.zeros(ab.n_traces, bool)
        sel[lst] = True
        g = orc.span_graph(ab.trace, ab.podop, ab.span, ab.parent, sel).as_graph()
        w.pr[anomaly] = orc.weights(g, orc.power_iteration(g, orc.preference(g, orc.trace_kinds(g), anomaly)))
    a_nodes, n_nodes = set(w.pr[True][0]), set(w.pr[False][0])
    w.Na, w.Nn, w.NP = len(a_nodes), len(n_nodes), ab.n_podops
    w.a_only, w.n_only, w.union = len(a_nodes - n_nodes), len(n_nodes - a_nodes), len(a_nodes | n_nodes)
    assert w.a_only > 0 and w.n_only > 0, name
    assert (w.Na, w.Nn, w.a_only, w.n_only, w.NP) == MEASURED[name], name
    w.one_block = fits(w.Na, w.Nn, w.NP, K)
    if name == "small":
        assert w.one_block and w.union > K
    if name == "mid":   # the widest network, and runs of more than one normal node per thread
        assert w.one_block and w.Nn > WS_T and w.union > 2048
    if name == "over":
        assert not w.one_block and w.NP <= WS_PMAX and w.Na + w.Nn > WS_MAX and w.union <= 4096
    if name == "big":   # off the one-block route by its pod-ops too; the general route's radix sort
        assert not w.one_block and w.NP > WS_PMAX and w.union > 4096
    return w


@functools.lru_cache(maxsize=None)
def oracle_spectrum(name, method):
    """The oracle's FULL spectrum result of the window: (codes, scores) in its order."""
    w = window(name)
    with np.errstate(all="ignore"):
        top, score, _ = orc.spectrum(w.pr[True][0], w.pr[False][0], w.n_normal, w.n_abnormal, w.union, w.pr[False][1],
                                     w.pr[True][1], method)
    assert len(top) == w.union and not np.isnan(np.array(score, np.float64)).any()
    return [int(c) for c in top], np.array(score, np.float64)


def rel_gt(a, b, tol):
    """|a - b| exceeds tol relative."""
    return abs(a - b) > tol * max(abs(a), abs(b))


def clusters(score, tol):
    """The oracle's ranks cut into runs [a, b) wherever two neighbours differ by more than tol
    relative: within a run the order is not defined at the tolerance, across a cut it is."""
    out, a = [], 0
    for i in range(1, len(score) + 1):
        if i == len(score) or rel_gt(score[i - 1], score[i], tol):
            out.append((a, i))
            a = i
    return out


def separated_ranks(score, tol, upto):
    """The ranks < upto whose oracle score differs from both neighbours by more than tol relative."""
    return [a for a, b in clusters(score, tol) if b == a + 1 and a < upto]


# The coverage-dominated formulas: a normal-only node has ef = nf = 1e-7 and np = Nl - n_num, an
# integer in the hundreds or thousands, so tarantula's ep / (ep + np) and the (ef + np) numerator of
# m1, hamann, simplematcing and rogers depend on the node's coverage alone up to its weight's
# (1 + w) * n_num: the normal-only nodes of equal coverage lead these rankings within 1e-8 or less of
# each other, by construction and on every seed (measured on 600-op windows of seeds 30..41: 0 to 9
# of the first 11 ranks separated for m1, 0 to 7 for the other four; on the four windows here 7 / 5 /
# 3 / 0 for m1 and 1 / 0 / 0 / 0 or less for the others, with gaps down to exactly 0).  For them the
# runs of near-equal ranks are compared as sets instead (check_against_oracle's last rule).
COVERAGE_TIED = ("m1", "tarantula", "hamann", "simplematcing", "rogers")


def check_against_oracle(name, method, codes, scores, *, rtol=1e-10, ranks=None):
    """A device result against the oracle's, with the PageRank weights agreeing only to ~rtol (the
    order of near-equal scores is not defined):
    * each returned code's score within rtol of the oracle's score for that code;
    * the returned scores non-increasing;
    * every oracle node whose score exceeds the last returned score by more than 10 rtol is returned;
    * for every run of oracle ranks that differs from both its neighbours by more than 100 rtol and
      lies within the returned entries, the returned codes on those ranks are the oracle's codes of
      those ranks as a set -- for a run of one rank (a rank separated from both neighbours): the
      code equals the oracle's code at that rank.
    ranks: only the first so many entries (fp32).  Returns the ranks of the runs of one."""
    o_codes, o_scores = oracle_spectrum(name, method)
    w = window(name)
    n = len(codes) if ranks is None else ranks
    assert len(codes) == len(scores) == min(K, w.union) and n <= len(codes)
    by_code = dict(zip(o_codes, o_scores))
    assert len(set(codes.tolist())) == len(codes)
    for c, s in zip(codes[:n].tolist(), scores[:n].tolist()):
        assert c in by_code, (name, method, c)
        assert not rel_gt(s, by_code[c], rtol), (name, method, c, s, by_code[c])
    assert (np.diff(scores[:n]) <= 0).all(), (name, method)
    if ranks is None:
        last, got = float(scores[-1]), set(codes.tolist())
        for c, s in zip(o_codes, o_scores):
            if s > last and rel_gt(s, last, 10 * rtol):
                assert c in got, (name, method, c, s, last)
    single = []
    for a, b in clusters(o_scores, 100 * rtol):
        if b > n:
            break
        assert sorted(codes[a:b].tolist()) == sorted(o_codes[a:b]), (name, method, a, b)
        if b == a + 1:
            single.append(a)
    return single


# ---------------------------------------------------------------- device side
class Dev:
    """The windows' tables on the device and the entry points' argument forms."""

    def __init__(self):
        from microrank_amd import _lib
        from microrank_amd.preprocess_data import DeviceSpans

        self.ctx = _lib.default_context()
        self.devs = {}
        for name in WINDOWS:
            self.devs[name] = DeviceSpans(self.ctx, window(name).table)

    def close(self):
        for d in self.devs.values():
            d.close()

    def win(self, name):
        w = window(name)
        return (self.devs[name], w.t0, w.t1, w.a3, w.ok)

    def batch(self, names, method, top_max=250, precision="fp64"):
        """rank_windows over the named windows: [(codes, scores)], counts and statuses checked."""
        from microrank_amd.online_rca import rank_windows

        got = rank_windows(self.ctx, [self.win(nm) for nm in names], top_max=top_max, spectrum_method=method,
                           precision=precision)
        for nm, r in zip(names, got):
            assert r[5] == 0 and (r[2], r[3]) == (window(nm).n_abnormal, window(nm).n_normal), nm
        return [(r[0], r[1]) for r in got]

    def single(self, name, method, top_max=250):
        """rca_window on the resident table: (codes, scores)."""
        import pandas as pd

        from microrank_amd.online_rca import rca_window

        w = window(name)
        out = rca_window(None, pd.Timestamp(w.t0), pd.Timestamp(w.t1), w.slo, top_max=top_max, spectrum_method=method,
                         ctx=self.ctx, table=w.table, dev=self.devs[name])
        assert (out["n_abnormal"], out["n_normal"]) == (w.n_abnormal, w.n_normal)
        names = w.table.podop_names
        top = out["top"]
        if names is not None:
            code_of = {nm: c for c, nm in enumerate(names)}
            assert len(code_of) == len(names)
            top = [code_of[nm] for nm in top]
        return np.array(top, np.int32), np.array(out["score"], np.float64)


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


KNOBS = ("MR_NO_WIN_SPECTRUM_SMALL", "MR_NO_LO_WIN")


def same(a, b):
    return list(a[0]) == list(b[0]) and a[1].tobytes() == b[1].tobytes()


def close_to(a, b, rtol=1e-12):
    """A window ranked in another batch: the PageRanks of a group share launches, and a window's
    weights can differ in the last bits with the group's other windows (measured: scores 1e-15 to
    1.2e-14 relative apart when the 5200-op window joins the batch, bitwise otherwise) -- the
    project's batch-against-standalone tolerance of 1e-12 (test_windows_batch_matches_standalone):
    the sorted scores agree rank by rank, and the codes agree as sets over every run of ranks cut
    where neighbours differ by more than 100 rtol (so exactly at every separated rank; but for the
    last run of a list of K, which may go on past the returned entries)."""
    if len(a[0]) != len(b[0]) or not np.allclose(a[1], b[1], rtol=rtol, atol=0):
        return False
    runs = clusters(b[1], 100 * rtol)
    if len(b[0]) >= K:
        runs = runs[:-1]
    return all(sorted(a[0][lo:hi].tolist()) == sorted(b[0][lo:hi].tolist()) for lo, hi in runs)


def test_windows_have_nodes_on_both_sides():
    """The docstring's table (CPU side only; every test below relies on it)."""
    for name in WINDOWS:
        w = window(name)
        assert w.n_abnormal > 0 and w.n_normal > 0
    assert [window(nm).one_block for nm in ("small", "mid", "over", "big")] == [True, True, False, False]


def test_oracle_ranks_are_separated():
    """The cap on the ranks whose code the oracle comparison cannot pin: at least 90 % of the first
    11 ranks are separated (by more than 1e-8 relative) in the oracle, on every window, for the
    eight formulas led by anomaly-side nodes (measured: 11 of 11 everywhere).  The five
    coverage-dominated formulas (COVERAGE_TIED) cannot meet it on any window with normal-only nodes;
    their runs of near-equal ranks are compared as sets, and here at least the small window's first
    11 ranks must fall into runs that end inside the returned 256."""
    for name in WINDOWS:
        for m in METHODS:
            sep = separated_ranks(oracle_spectrum(name, m)[1], 1e-8, 11)
            if m not in COVERAGE_TIED:
                assert len(sep) >= 0.9 * 11, (name, m, sep)
    for m in COVERAGE_TIED:
        runs = [r for r in clusters(oracle_spectrum("small", m)[1], 1e-8) if r[1] <= K]
        assert runs and runs[0][0] == 0 and max(b for _, b in runs) >= 11 and len(runs) >= 80, m


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_window_routes_agree_bitwise(method, dev, monkeypatch):
    """The small, the 2100-op and the 5200-op window through rca_window (one window), rank_windows
    (each alone; the two that fit together: two blocks of k_win_spectrum_b; the three together, the
    5200-op one on the general route beside them) and rank_windows under MR_NO_WIN_SPECTRUM_SMALL=1
    (k_union_* + mr_spectrum_dev), K = 256.  Codes and score bytes are equal wherever the windows'
    PageRanks ran in the same launches: rca_window and the window alone, the two that fit alone
    and together, and either spectrum route over one batch.  (The three together against each
    alone: see close_to.)  And k_win_spectrum itself, which a window alone reaches on the general
    window build (MR_NO_LO_WIN=1): bitwise the general spectrum route on that build."""
    names = ("small", "mid", "big")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    one = [dev.single(nm, method) for nm in names]
    alone = [dev.batch((nm,), method)[0] for nm in names]
    pair = dev.batch(names[:2], method)
    trio = dev.batch(names, method)
    monkeypatch.setenv("MR_NO_WIN_SPECTRUM_SMALL", "1")
    alone_general = [dev.batch((nm,), method)[0] for nm in names]
    trio_general = dev.batch(names, method)
    for i, nm in enumerate(names):
        assert len(alone[i][0]) == K, nm
        assert same(one[i], alone[i]), (nm, "rca_window / rank_windows")
        assert same(alone[i], alone_general[i]), (nm, "one block / general, alone")
        assert same(trio[i], trio_general[i]), (nm, "one block / general, batch of three")
        assert close_to(trio[i], alone[i]), (nm, "batch of three / alone")
        if i < 2:
            assert same(pair[i], alone[i]), (nm, "batch of two / alone")
    monkeypatch.setenv("MR_NO_LO_WIN", "1")
    gen_build = [dev.single(nm, method) for nm in names[:2]]
    monkeypatch.delenv("MR_NO_WIN_SPECTRUM_SMALL")
    one_block = [dev.single(nm, method) for nm in names[:2]]
    for nm, a, b in zip(names, one_block, gen_build):
        assert len(a[0]) == K and same(a, b), (nm, "k_win_spectrum / general, general window build")


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_window_spectrum_against_oracle(method, dev, monkeypatch):
    """Every window's default route against oracle.spectrum fed from the oracle's own window
    (detector, graphs, PageRanks): an error shared by all routes -- a wrong formula, a wrong A / Nl
    (T1) -- shows here.  fp64 at the project's window tolerance of 1e-10 (check_against_oracle)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    names = tuple(WINDOWS)
    for nm, (codes, scores) in zip(names, dev.batch(names, method)):
        single = check_against_oracle(nm, method, codes, scores)
        if method not in COVERAGE_TIED:   # (test_oracle_ranks_are_separated: the rank rule pins the top)
            assert len([r for r in single if r < 11]) >= 0.9 * 11, (nm, method)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dstar2", "ochiai"])
def test_window_spectrum_against_oracle_fp32(method, dev, monkeypatch):
    """precision="fp32": the first five ranks at 1e-4."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    names = tuple(WINDOWS)
    for nm, (codes, scores) in zip(names, dev.batch(names, method, precision="fp32")):
        check_against_oracle(nm, method, codes, scores, rtol=1e-4, ranks=5)


@pytest.mark.gpu
def test_windows_off_the_one_block_route(dev, monkeypatch):
    """Na + Nn > 4096 with NP <= 4096 ("over") and NP > 4096 with a union above 4096 ("big": the
    radix sort inside a window) take the general route by default: bitwise the explicit
    MR_NO_WIN_SPECTRUM_SMALL=1 run, alone and as a batch of the two, for a formula of each sign
    pattern.  (Their oracle comparison: test_window_spectrum_against_oracle.)"""
    for method in ("dstar2", "goodman", "tarantula"):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        default = [dev.batch((nm,), method)[0] for nm in ("over", "big")]
        both = dev.batch(("over", "big"), method)
        monkeypatch.setenv("MR_NO_WIN_SPECTRUM_SMALL", "1")
        explicit = [dev.batch((nm,), method)[0] for nm in ("over", "big")]
        both_explicit = dev.batch(("over", "big"), method)
        for i, nm in enumerate(("over", "big")):
            assert len(explicit[i][0]) == K
            assert same(default[i], explicit[i]) and same(both[i], both_explicit[i]), (nm, method)
            assert close_to(both[i], default[i]), (nm, method)


@pytest.mark.gpu
def test_top_list_longer_than_the_one_block_route_holds(dev, monkeypatch):
    """top_max = 251 (K = 257 > WS_KMAX) on the small window: 257 entries (its union is larger), the
    first 256 bitwise those of top_max = 250, through rank_windows and rca_window."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert window("small").union >= 257 and not fits(window("small").Na, window("small").Nn, window("small").NP, 257)
    for method in ("dstar2", "hamann"):
        for run in (lambda tm: dev.batch(("small",), method, top_max=tm)[0], lambda tm: dev.single("small", method, tm)):
            a, b = run(250), run(251)
            assert len(a[0]) == 256 and len(b[0]) == 257
            assert list(b[0][:256]) == list(a[0]) and b[1][:256].tobytes() == a[1].tobytes()
            assert b[1][256] <= b[1][255]
            by_code = dict(zip(*oracle_spectrum("small", method)))
            assert not rel_gt(float(b[1][256]), by_code[int(b[0][256])], 1e-10)


@pytest.mark.gpu
def test_batch_mixing_routes_equals_windows_alone(dev, monkeypatch):
    """A batch of a window that fits the one-block route and one that does not (in both orders,
    and with the 2100-op window between them): the windows' results land in their own places --
    bitwise those of the same batch with every window on the general route, and each window's result
    that of the window ranked alone (close_to: its PageRanks ran in other launches)."""
    for method in ("dstar2", "rogers"):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        alone = {nm: dev.batch((nm,), method)[0] for nm in ("small", "mid", "over")}
        combos = (("small", "over"), ("over", "small"), ("over", "mid", "small", "over"))
        mixed = [dev.batch(names, method) for names in combos]
        monkeypatch.setenv("MR_NO_WIN_SPECTRUM_SMALL", "1")
        for names, got in zip(combos, mixed):
            general = dev.batch(names, method)
            for nm, g, e in zip(names, got, general):
                assert same(g, e), (names, nm, method)
                assert close_to(g, alone[nm]), (names, nm, method)
