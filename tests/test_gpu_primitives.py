"""The shared device primitives alone, against numpy and Python integers, at the sizes where their paths
change: the exclusive scan (mr_prim.hip), the radix sort (mr_sort.hip), wave_run_reduce, the block
reductions and block_owner (mr_prim.h), EvRun / EvTable (mr_evidence.h).  They run through the test-only
library of tests/csrc/mr_selftest.hip (prim_util.py); every comparison is exact."""
import math

import numpy as np
import pytest

import prim_util as pu
from microrank_amd import _lib

pytestmark = pytest.mark.gpu

T = pu.SCAN_TILE


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


# ---------------------------------------------------------------- scan
# one block up to 16384 (two rounds of its 8192 past 8192); look-back tiles of 2048 beyond: 9 tiles, 64
# and 65 (a tile whose predecessors fill one poll exactly), 66 and 201 (a second, a fourth poll)
SCAN_SIZES = [0, 1, 2, 63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385, T * 64, T * 64 + 1, T * 65 + 1, T * 200 + 17]


def _scan_inputs(n, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 9, n) * (rng.random(n) < 0.3)   # many zeros
    return {"random": counts, "zeros": np.zeros(n, np.int64), "ones": np.ones(n, np.int64)}


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizes(ctx, n):
    for name, a in _scan_inputs(n, 1000 + n).items():
        ref = pu.ref_scan(a)
        assert ref[n] == a.sum()
        for dtype, in_place in ((np.int64, False), (np.int64, True), (np.int32, False)):
            got = pu.scan(ctx, a.astype(dtype), in_place=in_place)
            assert np.array_equal(got, ref), (name, dtype.__name__, in_place, int(np.flatnonzero(got != ref)[0]))


def test_scan_status_words_grow(ctx):
    """16.8M int32 counts need 8193 status words: the context's words are freed and allocated again
    between two look-back scans that use the first 65 of them."""
    rng = np.random.default_rng(7)
    small = rng.integers(0, 5, T * 64 + 1).astype(np.int64)
    assert np.array_equal(pu.scan(ctx, small), pu.ref_scan(small))
    assert pu.scan_state(ctx)[1] == pu.SCAN_WORDS_MIN
    n = T * 8192 + 5
    big = rng.integers(0, 4, n, dtype=np.int32)
    got = pu.scan(ctx, big)
    ref = pu.ref_scan(big)
    assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
    assert pu.scan_state(ctx) == (1, 8193)   # (new words: the epochs start over)
    assert np.array_equal(pu.scan(ctx, small), pu.ref_scan(small))
    assert np.array_equal(pu.scan(ctx, small, in_place=True), pu.ref_scan(small))


def test_scan_lookback_total_just_below_2_42(ctx):
    """The look-back words carry 42 value bits: every tile's inclusive prefix up to 2^42 - 1 must pass
    (a total of 2^42 or more on this path is outside the documented limit, and not tested)."""
    n = T * 70 + 3
    rng = np.random.default_rng(42)
    a = rng.integers(0, 1000, n).astype(np.int64)
    a[0] += (1 << pu.DL_VB) - 1 - a.sum()   # (in the first tile: every published prefix is near the limit)
    ref = pu.ref_scan(a)
    assert ref[n] == (1 << 42) - 1
    for in_place in (False, True):
        assert np.array_equal(pu.scan(ctx, a, in_place=in_place), ref)


@pytest.mark.parametrize("n", [1000, 8192, 8193, 16384])
def test_scan_single_block_is_full_int64(ctx, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 1 << 48, n).astype(np.int64)
    ref = pu.ref_scan(a)
    assert ref[n] > (1 << 42)
    assert np.array_equal(pu.scan(ctx, a), ref) and np.array_equal(pu.scan(ctx, a, in_place=True), ref)


def test_scan_epoch_wrap():
    """After 2^20 look-back scans on a context the 20-bit epoch comes back to 1, where the status words
    still hold flag-2 words of epoch 1: the first call's prefixes.  Only the clear at the wrap keeps the
    second epoch-1 call from taking them for its own (a wrong prefix, not a wait)."""
    c = _lib.Context()
    try:
        rng = np.random.default_rng(20)
        n = T * 200
        x = rng.integers(500, 1000, n).astype(np.int64)
        y = rng.integers(0, 4, n).astype(np.int32)
        assert np.array_equal(pu.scan(c, x), pu.ref_scan(x))
        assert pu.scan_state(c) == (1, pu.SCAN_WORDS_MIN)
        pu.set_scan_epoch(c, (1 << pu.DL_EB) - 1)
        got = pu.scan(c, y)
        assert pu.scan_state(c) == (1, pu.SCAN_WORDS_MIN)   # the same words, epoch 1 again
        ref = pu.ref_scan(y)
        assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
        for m in (T * 65 + 1, T * 200 + 17):
            z = rng.integers(0, 7, m).astype(np.int64)
            assert np.array_equal(pu.scan(c, z, in_place=True), pu.ref_scan(z))
        assert pu.scan_state(c)[0] == 3
    finally:
        c.close()


# ---------------------------------------------------------------- sort
# LDS bitonic sort up to 4096 (padded to a power of two); radix tiles of 2048 beyond: 3 tiles, 3 tiles and
# a key, 65 tiles (the histogram scan of 256 * 65 counts takes the look-back path), 147 tiles
SORT_SMALL = [0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145]
SORT_LARGE = [T * 64 + 1, 300_007]
SORT_BITS = [1, 7, 8, 9, 16, 17, 24, 32, 33, 46, 63, 64]
SORT_BITS_LARGE = [1, 9, 16, 33, 63, 64]   # odd and even pass counts, partial last digits


def _sort_keys(n, bits, seed):
    rng = np.random.default_rng(seed)
    full = rng.integers(0, 1 << 64, n, dtype=np.uint64)   # garbage above `bits`
    by_mask = full[pu.ref_sort_perm(full, bits)] if n else full
    few = rng.integers(0, 1 << 64, 5, dtype=np.uint64)
    return {
        "random": full,
        "equal": np.full(n, few[0], np.uint64),
        "two": np.where(rng.random(n) < 0.5, few[1], few[1] ^ np.uint64(1)),
        "sorted": by_mask,
        "reversed": by_mask[::-1].copy(),
        "few": few[rng.integers(0, 5, n)],
    }


def _check_sort(ctx, keys, bits, what):
    n = keys.size
    perm = pu.ref_sort_perm(keys, bits)
    vals = np.arange(n, dtype=np.uint32)   # the input position: stability shows
    k, v = pu.sort(ctx, keys, vals, bits)
    assert np.array_equal(k, keys[perm]), (what, "keys with vals")   # all 64 bits ride along
    assert np.array_equal(v, vals[perm]), (what, "vals")
    k, _ = pu.sort(ctx, keys, None, bits)
    assert np.array_equal(k, keys[perm]), (what, "keys alone")


@pytest.mark.parametrize("n", SORT_SMALL)
def test_sort_sizes(ctx, n):
    for bits in SORT_BITS:
        for name, keys in _sort_keys(n, bits, 31 * n + bits).items():
            _check_sort(ctx, keys, bits, (name, bits))


@pytest.mark.parametrize("n", SORT_LARGE)
def test_sort_large(ctx, n):
    for bits in SORT_BITS_LARGE:
        pats = _sort_keys(n, bits, 31 * n + bits)
        for name in ("random", "few") if bits not in (9, 64) else pats:
            _check_sort(ctx, pats[name], bits, (name, bits))


@pytest.mark.parametrize("n", [3, 1025, 4095, 4097, 6145])
def test_sort_keys_equal_to_the_padding_value(ctx, n):
    """The LDS path fills its power of two with ~0 keys behind the input: real ~0 keys stay in input
    order ahead of them (and the radix sizes agree)."""
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    keys[rng.random(n) < 0.4] = np.uint64(pu.M64)
    keys[n - 1] = np.uint64(pu.M64)
    _check_sort(ctx, keys, 64, "~0 keys")
    _check_sort(ctx, np.full(n, pu.M64, np.uint64), 64, "all ~0")


# ---------------------------------------------------------------- wave_run_reduce
def _run_streams():
    """name -> (keys, has, d): non-negative keys (the filler of a last partial wave is -1)."""
    rng = np.random.default_rng(5)
    B = pu.EV_BIAS

    def vals(n):
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)

    def by_lengths(lens, distinct=True):
        ks = np.arange(len(lens)) if distinct else rng.integers(0, 3, len(lens))
        return np.repeat(ks, lens)

    out = {}
    k = np.full(192, 11)
    out["one key over whole waves"] = (k, np.ones(192, bool), vals(192))
    k = rng.permutation(256)
    out["all distinct"] = (k, np.ones(256, bool), vals(256))
    k = np.tile([3, 8], 96)
    out["ABAB"] = (k, np.ones(192, bool), vals(192))
    k = np.concatenate([np.arange(60), [77] * 4, [77] * 5, np.arange(100, 159)])
    out["a key in lane 63 and the next lane 0"] = (k, np.ones(128, bool), vals(128))
    k = by_lengths(np.arange(1, 31))   # 465 lanes: runs cut by wave ends, a partial last wave
    out["lengths 1, 2, 3, ..."] = (k, np.ones(k.size, bool), vals(k.size))
    k = by_lengths(rng.integers(1, 40, 60), distinct=False)   # (equal neighbours merge: still runs)
    out["random lengths"] = (k, np.ones(k.size, bool), vals(k.size))
    k = by_lengths(rng.integers(1, 12, 80))
    has = rng.random(k.size) < 0.6
    has[np.flatnonzero(np.diff(k, prepend=-1))[::2]] = False   # every other run is headed by a lane without a value
    out["lanes without a value"] = (k, has, vals(k.size))
    k = by_lengths(rng.integers(1, 70, 12))
    near = rng.integers(0, 7, k.size).astype(np.uint64) + np.uint64(B - 3)   # around 2^63: sums wrap, the bias flips
    out["values near 2^63"] = (k, np.ones(k.size, bool), near)
    out["a partial wave alone"] = (np.array([4, 4, 9]), np.ones(3, bool), vals(3))
    k = np.repeat([5, 5 + (1 << 32), 5, 5 + (1 << 33)], [20, 20, 30, 40])
    out["keys that differ above bit 31"] = (k, np.ones(k.size, bool), vals(k.size))
    return out


RUN_STREAMS = _run_streams()


@pytest.mark.parametrize("name", list(RUN_STREAMS))
def test_wave_run_reduce(ctx, name):
    keys, has, d = RUN_STREAMS[name]
    widths = (64,) if keys.max() >= (1 << 31) else (32, 64)
    for key_bits in widths:
        for off in (0, 1 << 40) if key_bits == 64 else (0,):   # (64-bit keys: all of the key is compared)
            ref = pu.ref_runs(keys + off, has, d)
            got = pu.runs(ctx, key_bits, keys + off, has, d)
            for what, g, r in zip(("n", "sum", "max", "last"), got, ref):
                assert np.array_equal(g, r), (key_bits, off, what, int(np.flatnonzero(g != r)[0]))
            # exactly one flagged lane per run, and it holds the whole run
            assert int(got[3].sum()) == sum(
                int(np.count_nonzero(np.diff(w)) + 1) for w in np.array_split(keys, np.arange(64, keys.size, 64)))


# ---------------------------------------------------------------- EvTable
def _ev_rows(rng, pool, n, gaps=0.1):
    """n rows over the keys of `pool` in runs of 1..6 (what the evidence kernels see), some rows without a key."""
    ks = np.repeat(rng.choice(pool, n), rng.integers(1, 7, n))[:n]
    ks[rng.random(n) < gaps] = -1
    return ks.astype(np.int64), rng.integers(0, 1 << 64, n, dtype=np.uint64)


def _colliding(slot, count, start=1):
    out, k = [], start
    while len(out) < count:
        if pu.ev_hash(k) == slot:
            out.append(k)
        k += 1
    return out


def _ev_cases():
    rng = np.random.default_rng(9)
    cases = {}
    keys, d = _ev_rows(rng, np.arange(pu.EV_H), 20000)
    cases["direct"] = (True, keys, d, pu.EV_H, 5, 16)
    keys, d = _ev_rows(rng, np.arange(300), 3000)
    cases["direct, one block, few keys"] = (True, keys, d, 300, 1, 12)
    pool = rng.permutation(6000)[:5000]
    keys, d = _ev_rows(rng, pool, 40000)
    assert np.unique(keys[keys >= 0]).size > pu.EV_H
    cases["hashed, 5000 keys"] = (False, keys, d, 6000, 7, 23)
    same = _colliding(pu.ev_hash(12345), 12)
    assert len({pu.ev_hash(k) for k in same}) == 1
    keys, d = _ev_rows(rng, np.array(same), 6000)
    cases["hashed, one slot"] = (False, keys, d, max(same) + 1, 3, 8)
    zero = [0] + _colliding(0, 2) + [7]   # key 0 is stored as 1; two more keys want its slot
    keys, d = _ev_rows(rng, np.array(zero), 4000)
    cases["hashed, key 0"] = (False, keys, d, max(zero) + 1, 4, 4)
    cases["hashed, key 0 alone"] = (False, np.zeros(700, np.int64), d[:700], 1, 2, 2)
    return cases


EV_CASES = _ev_cases()


@pytest.mark.parametrize("name", list(EV_CASES))
def test_evtable(ctx, name):
    direct, keys, d, n_keys, blocks, tiles = EV_CASES[name]
    ref = pu.ref_evtable(keys, d, n_keys)
    for key_bits in (32, 64):
        a = pu.evtable(ctx, key_bits, direct, keys, d, n_keys, blocks, tiles)
        b = pu.evtable(ctx, key_bits, direct, keys, d, n_keys, blocks, tiles)
        assert np.array_equal(a, ref), (key_bits, np.argwhere(a != ref)[0].tolist())
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- block reductions
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("block", [64, 256, 1024])
def test_block_and_wave_sums(ctx, block):
    rng = np.random.default_rng(block)
    n = 3 * block
    v = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)   # both signs, sixty binades: the order shows
    for op in ("block_sum", "wave_sum"):
        got = pu.block_reduce(ctx, op, block, v)
        assert np.array_equal(_bits(got), _bits(pu.ref_block_reduce(op, block, v))), op
        span = block if op == "block_sum" else 64
        for s0 in range(0, n, span):
            seg = v[s0:s0 + span]
            assert len(set(_bits(got[s0:s0 + span]).tolist())) == 1   # every thread holds the same bits
            assert abs(float(got[s0]) - math.fsum(seg)) <= span * 2.0**-53 * math.fsum(np.abs(seg))
    iv = rng.integers(-(1 << 62), 1 << 62, n)   # (sums wrap)
    got = pu.block_reduce(ctx, "wave_sum_i64", block, iv)
    assert np.array_equal(got, np.repeat(iv.reshape(-1, 64).sum(axis=1), 64))
    assert np.array_equal(got, pu.ref_block_reduce("wave_sum_i64", block, iv))


@pytest.mark.parametrize("block", [64, 256, 1024])
def test_block_and_wave_maxima(ctx, block):
    rng = np.random.default_rng(block + 1)
    inf, nan = float("inf"), float("nan")
    plain = rng.standard_normal(block)
    neg = np.full(block, -inf)
    one = neg.copy()
    one[block - 1] = -5.0
    with_nan = plain.copy()
    with_nan[block // 2 + 3] = nan
    nan_inf = np.full(block, inf)
    nan_inf[block - 1] = nan
    v = np.concatenate([plain, neg, one, with_nan, nan_inf, -np.abs(plain)])
    for op, span in (("block_max", block), ("wave_max", 64)):
        got = pu.block_reduce(ctx, op, block, v)
        for s0 in range(0, v.size, span):
            seg, g = v[s0:s0 + span], got[s0:s0 + span]
            if np.isnan(seg).any():
                assert np.isnan(g).all(), (op, s0)   # a NaN anywhere gives NaN
            else:
                assert np.array_equal(_bits(g), _bits(np.full(span, seg.max()))), (op, s0)
        ref = pu.ref_block_reduce(op, block, v)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~np.isnan(got)], ref[~np.isnan(ref)])


# ---------------------------------------------------------------- block_owner
@pytest.mark.parametrize("first,n_blocks", [
    ([0], 5),                                    # a single descriptor
    ([0, 0, 3, 3, 3, 10], 12),                   # repeated starts: the last of equal starts owns
    ([0, 1], 2),
    ([0, 0, 0, 0], 3),
    ([0, 4, 4, 9, 9], 9),                        # trailing descriptors without a block in the launch
])
def test_block_owner_small(ctx, first, n_blocks):
    got = pu.block_owner(ctx, first, n_blocks)
    assert np.array_equal(got, pu.ref_block_owner(first, n_blocks)), got.tolist()


def test_block_owner_many(ctx):
    rng = np.random.default_rng(3)
    for n in (2, 3, 64, 1000, 1001):
        first = np.concatenate([[0], np.cumsum(rng.integers(0, 6, n - 1) * (rng.random(n - 1) < 0.6))])
        n_blocks = int(first[-1]) + 4
        got = pu.block_owner(ctx, first, n_blocks)
        ref = pu.ref_block_owner(first, n_blocks)
        assert np.array_equal(got, ref)
        assert got[0] == np.flatnonzero(first == 0)[-1] and got[-1] == n - 1   # block 0, the last block
