"""Deterministic inputs of calculate_spectrum_without_delay_list (online_rca.py:33-152) for the
spectrum tests, and their expected results from the numpy oracle (oracle.spectrum, pinned to the
reference on these very inputs by tests/golden/spectrum_synth.json).

``spectrum_case(n, seed, typed)`` builds a union of ``n`` nodes from integer hashes only (no numpy
Generator: another numpy must not change the inputs the fixture's results belong to):

* about a third each of anomaly-only, both and normal-only nodes (n = 1: a normal-only node, n = 2:
  an anomaly-only and a both node, n = 3: one of each); anomaly_result and normal_result list their
  keys in two unrelated permutations, so the union order (anomaly keys, then the normal-only keys in
  normal order) is the order of neither;
* weights from 8 values and counts from 4, both drawn with halving probabilities, so the largest
  exact-tie group holds about n / 12 nodes (hundreds at n = 4097) spread over the whole position
  range;
* edge nodes (n >= 4 where the kinds exist, asserted from n = 64): anomaly-only nodes with
  a_num = 0 (ef = +0); "both" nodes with a_num == A and n_num == 0 (ep + nf == 0: inf for dstar2 and
  m1 with a numpy-typed weight); a "both" node with the anomaly weight -0.0 and n_num >= 1 (ef = -0.0:
  a -0.0 score for jaccard, sorensendice, m2, russellrao and dice, tying with the +0.0 scores).

``typed``: "np" every weight np.float64; "mixed" about 1 in 7 weights a Python float, never both
weights of an ep + nf == 0 node (no Python-typed zero division); "zd_last" as "mixed", with the
union's LAST node (position n - 1) an all-Python "both" node with ep + nf == 0, so the reference
raises ZeroDivisionError for dstar2 and m1 only.  The union's last node can only be an anomaly key
when no normal-only node follows it, so the nodes "zd_last" would have made normal-only are "both".

NaN is out of scope (Python's sort of NaN keys is no defined order) and no case yields one -- with
one forced exception to the node list above: a zero anomaly weight makes ef = nf = 0, and then
ochiai's ef / sqrt((ep + ef) * (ef + nf)) and tarantula's ef / (ef + nf) are 0 / 0 whatever the
other values are.  A -0.0 score needs ef = -0.0 with a positive denominator, which only a zero
weight gives, so for these two methods the -0.0 node takes an ordinary weight (``neg_zero=False``,
what ``case_for`` passes for them).  ``expected`` asserts the absence of NaN on the oracle's full
result of every (case, method) it hands out.
"""
import functools
import math

import numpy as np

import oracle as orc

METHODS = orc.SPECTRUM_METHODS
A_LEN, N_LEN = 40, 37                       # anomaly_list_len, normal_list_len
WEIGHTS = (0.031, 0.023, 0.016, 0.011, 0.007, 0.004, 0.0025, 0.001)
A_COUNTS = (11, 3, 26, A_LEN)
N_COUNTS = (9, 21, 2, 0)
NO_NEG_ZERO = ("ochiai", "tarantula")       # 0 / 0 for a zero anomaly weight (module docstring)
SEED = 20260

_M = (1 << 64) - 1


def _h(seed, i, salt):
    """splitmix64 of (seed, i, salt)."""
    z = (seed * 0x9E3779B97F4A7C15 + i * 0xBF58476D1CE4E5B9 + salt * 0x94D049BB133111EB + 0x1234567) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def _halving(h, k):
    """0 .. k - 1 with probabilities 1/2, 1/4, .., the last two equal."""
    for j in range(k - 1):
        if (h >> j) & 1:
            return j
    return k - 1


AONLY, BOTH, NONLY = 0, 1, 2


def spectrum_case(n, seed=SEED, typed="np", neg_zero=True):
    """(anomaly_result, normal_result, anomaly_num_list, normal_num_list, anomaly_list_len,
    normal_list_len) for a union of ``n`` nodes (module docstring)."""
    assert n >= 1 and typed in ("np", "mixed", "zd_last")
    zd = typed == "zd_last"
    if n < 3:
        kind = {1: [NONLY], 2: [AONLY, BOTH]}[n]
    else:
        kind = [AONLY, BOTH, NONLY] + [_h(seed, i, 1) % 3 for i in range(3, n)]
    if zd:
        kind = [BOTH if k == NONLY else k for k in kind]
        kind[n - 1] = BOTH
    name = [f"p{i % 7}_op{i:05d}" for i in range(n)]
    a_w, n_w, a_c, n_c = [None] * n, [None] * n, [None] * n, [None] * n
    for i in range(n):
        if kind[i] != NONLY:
            a_w[i] = WEIGHTS[_halving(_h(seed, i, 2), 8)]
            a_c[i] = A_COUNTS[_halving(_h(seed, i, 3), 4)]
        if kind[i] != AONLY:
            n_w[i] = WEIGHTS[_halving(_h(seed, i, 4), 8)]
            n_c[i] = N_COUNTS[_halving(_h(seed, i, 5), 4)]
        if kind[i] == BOTH and a_c[i] == 3 and n_c[i] == 0 and _h(seed, i, 6) % 4:
            a_c[i] = A_LEN   # (more ep + nf == 0 nodes than the product of the two draws gives)
    py = [[False, False] for _ in range(n)]   # Python-typed (anomaly weight, normal weight)
    if typed != "np":
        for i in range(n):
            py[i] = [_h(seed, i, 7) % 7 == 0, _h(seed, i, 8) % 7 == 0]

    def first(k, start):
        return next((i for i in range(start, n - (1 if zd else 0)) if kind[i] == k), None)

    # edge nodes: the first node of the wanted kind from a given id on, and a sprinkling by hash
    if n >= 4:
        zero_ef = {first(AONLY, n // 5)} | {i for i in range(n) if kind[i] == AONLY and _h(seed, i, 9) % 41 == 0}
        for i in zero_ef - {None}:
            a_c[i] = 0
        i = first(BOTH, n // 3)
        if i is not None:
            a_c[i], n_c[i] = A_LEN, 0
        i = first(BOTH, n // 2)
        if i is not None:
            n_c[i] = 21
            py[i][0] = False
            if neg_zero:
                a_w[i] = -0.0
    for i in range(n):   # no Python-typed zero division in ep + nf (dstar2, m1) but the one asked for
        if kind[i] == BOTH and a_c[i] == A_LEN and n_c[i] == 0:
            py[i] = [False, False]
    if zd:
        i = n - 1
        a_w[i], n_w[i], a_c[i], n_c[i], py[i] = WEIGHTS[2], WEIGHTS[4], A_LEN, 0, [True, True]
    a_ids = sorted((i for i in range(n - (1 if zd else 0)) if kind[i] != NONLY), key=lambda i: _h(seed, i, 10))
    if zd:
        a_ids.append(n - 1)
    n_ids = sorted((i for i in range(n) if kind[i] != AONLY), key=lambda i: _h(seed, i, 11))
    typ = lambda v, p: float(v) if p else np.float64(v)
    anomaly_result = {name[i]: typ(a_w[i], py[i][0]) for i in a_ids}
    normal_result = {name[i]: typ(n_w[i], py[i][1]) for i in n_ids}
    anomaly_num = {name[i]: a_c[i] for i in a_ids}
    normal_num = {name[i]: n_c[i] for i in n_ids}
    return anomaly_result, normal_result, anomaly_num, normal_num, A_LEN, N_LEN


def case_for(method, n, seed=SEED, typed="np"):
    return spectrum_case(n, seed, typed, neg_zero=method not in NO_NEG_ZERO)


def union(case):
    """The reference's node order: anomaly_result's keys, then normal_result's other keys."""
    a, nr = case[0], case[1]
    return list(a) + [k for k in nr if k not in a]


def run_oracle(case, method, top_max):
    a, nr, an, nn, A, N = case
    with np.errstate(all="ignore"):
        return orc.spectrum(a, nr, A, N, top_max, nn, an, method)


@functools.lru_cache(maxsize=None)
def expected(n, typed="np", seed=SEED):
    """{method: "ZeroDivisionError" | (names, scores, lines)}: the oracle's FULL sorted result
    (top_max = n - 6) of case_for(method, n, seed, typed), checked: no NaN anywhere; the union as
    described; from n = 64 the "np" case has an inf (dstar2) and a -0.0 (jaccard) score, "zd_last"
    raises for dstar2 and m1 only and its last union node is the all-Python one."""
    out = {}
    for m in METHODS:
        case = case_for(m, n, seed, typed)
        assert len(union(case)) == n
        try:
            top, score, lines = run_oracle(case, m, n - 6)
        except ZeroDivisionError:
            out[m] = "ZeroDivisionError"
            continue
        assert len(top) == n and not any(math.isnan(float(s)) for s in score), (n, typed, m)
        out[m] = (top, score, lines)
    case = spectrum_case(n, seed, typed)
    a, nr = case[0], case[1]
    if n >= 3 and typed != "zd_last":
        u = union(case)
        assert set(a) - set(nr) and set(a) & set(nr) and set(nr) - set(a)
        if n >= 64:   # neither input's order, nor the ids' order
            assert u != sorted(u) and [k for k in nr if k in a] != [k for k in a if k in nr]
    if typed == "zd_last":
        assert [m for m in METHODS if out[m] == "ZeroDivisionError"] == ["dstar2", "m1"]
        last = union(case)[-1]
        assert type(a[last]) is float and type(nr[last]) is float
    else:
        assert "ZeroDivisionError" not in out.values()
    if n >= 64 and typed == "np":
        assert any(math.isinf(float(s)) for s in out["dstar2"][1])
        assert any(float(s) == 0.0 and math.copysign(1.0, float(s)) < 0 for s in out["jaccard"][1])
        assert any(float(s) == 0.0 and math.copysign(1.0, float(s)) > 0 for s in out["jaccard"][1])
    if typed == "mixed" and n >= 64:
        kinds = {type(v) for v in list(a.values()) + list(nr.values())}
        assert kinds == {float, np.float64}
    return out


def largest_tie_group(scores):
    from collections import Counter

    return max(Counter(float(s) for s in scores).values())
