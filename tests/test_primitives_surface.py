"""CPU checks around the device-primitive tests (test_gpu_primitives.py): the test-only library is built,
loads without a GPU beside the one product library and exports what the loader declares; bits_for, which
runs on the host; and every Python reference on cases worked out by hand."""
import ctypes
import os

import numpy as np

import prim_util as pu
from microrank_amd import _lib

NAN, INF = float("nan"), float("inf")


def test_selftest_library_is_built_loads_and_exports_the_loader_names():
    assert os.path.exists(pu.SELFTEST_PATH), "libmicrorank_selftest.so not built (run __graft_entry__.build())"
    lib = pu.load()
    missing = [name for name in pu.SIGNATURES if not hasattr(lib, name)]
    assert not missing, missing
    assert all(name.startswith("mrt_") for name in pu.SIGNATURES)
    # the product library holds none of them, and is mapped once (the selftest library links against it)
    product = ctypes.CDLL(_lib.LIB_PATH)
    assert not [name for name in pu.SIGNATURES if hasattr(product, name)]
    with open("/proc/self/maps") as f:
        mapped = {line.split()[-1] for line in f if "libmicrorank_hip" in line}
    assert mapped == {os.path.realpath(_lib.LIB_PATH)}, mapped


def test_selftest_source_is_outside_the_product_sources():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mr_selftest.hip")
    text = open(src).read()
    assert os.path.exists(src) and '.hip"' not in text   # (it links the product's host functions, re-includes none)
    assert not os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "mr_selftest.hip"))


def test_bits_for():
    got = [pu.bits_for(v) for v in (0, 1, 2, 255, 256, 2**32 - 1, 2**32, 2**63, 2**64 - 1)]
    assert got == [0, 1, 2, 8, 9, 32, 33, 64, 64]


def test_ref_scan_and_sort_perm():
    assert pu.ref_scan(np.array([3, 0, 4], np.int32)).tolist() == [0, 3, 3, 7]
    assert pu.ref_scan(np.zeros(0, np.int64)).tolist() == [0]
    assert pu.ref_scan(np.array([2**31 - 1, 2**31 - 1, 1], np.int32)).tolist() == [0, 2**31 - 1, 2**32 - 2, 2**32 - 1]
    keys = np.array([0x103, 0x002, 0x203, 0x001], np.uint64)
    assert pu.ref_sort_perm(keys, 8).tolist() == [3, 1, 0, 2]     # 3, 2, 3, 1 under the mask: ties in input order
    assert pu.ref_sort_perm(keys, 64).tolist() == [3, 1, 0, 2]
    assert pu.ref_sort_perm(keys, 1).tolist() == [1, 0, 2, 3]     # 1, 0, 1, 1
    assert pu.ref_sort_perm(np.array([2**64 - 1, 2**63, 0], np.uint64), 64).tolist() == [2, 1, 0]


def test_ref_runs_by_hand():
    B = pu.EV_BIAS
    n, s, m, last = pu.ref_runs([5, 5, 7, 5], [1, 0, 1, 1], [10, 99, B, 3])
    assert n.tolist() == [1, 1, 1, 1]
    assert s.tolist() == [10, 10, B, 3]                 # lane 1 brings no value: its 99 does not count
    assert m.tolist() == [10 ^ B, 10 ^ B, 0, 3 ^ B]     # d = 2^63 is the smallest biased value
    assert last.tolist() == [0, 1, 1, 1]                # the two runs of 5 are not adjacent
    # a run that heads with a lane without a value, sums that wrap, a negative duration below a positive one
    n, s, m, last = pu.ref_runs([4, 4, 4], [0, 1, 1], [7, B + 5, B + 6])
    assert n.tolist() == [0, 1, 2] and s.tolist() == [0, B + 5, 11] and m.tolist() == [0, 5, 6]
    assert last.tolist() == [0, 0, 1]
    # one key over 65 lanes: the wave ends the run at lane 63, lane 64 starts over
    n, s, m, last = pu.ref_runs([9] * 65, [1] * 65, [1] * 65)
    assert n.tolist() == list(range(1, 65)) + [1] and s.tolist() == n.tolist()
    assert last.tolist() == [0] * 63 + [1, 1]
    # key -1 lanes (no row) form runs like any key, and fill the last wave
    n, s, m, last = pu.ref_runs([-1, -1, 2], [0, 0, 1], [0, 0, 8])
    assert n.tolist() == [0, 0, 1] and last.tolist() == [0, 1, 1]


def test_ev_hash_and_ref_evtable_by_hand():
    # 0x9E3779B97F4A7C15 = 1001 1110 0011 ...: its top ten bits are 10 0111 1000; twice it (mod 2^64) is
    # 0x3C6EF372FE94F82A = 0011 1100 0110 ...: 00 1111 0001
    assert pu.ev_hash(0) == 0 and pu.ev_hash(1) == 0b1001111000 and pu.ev_hash(2) == 0b0011110001
    assert pu.ev_hash(2**32) == (0x7F4A7C1500000000 >> 54)
    assert all(0 <= pu.ev_hash(k) < pu.EV_H for k in range(5000))
    B = pu.EV_BIAS
    cnt = pu.ref_evtable([2, -1, 0, 2, 2], [B, 77, 1, B, 2**64 - 1], 4)
    assert cnt.tolist() == [[1, 1, 1 ^ B], [0, 0, 0], [3, 2**64 - 1, (2**64 - 1) ^ B], [0, 0, 0]]   # (B + B wraps to 0)


def test_butterfly_and_block_reduce_by_hand():
    assert (pu.butterfly(np.arange(64, dtype=np.float64), "sum") == 2016.0).all()
    # the order shows: 1 meets lane 32's 2^-53 first (1 + 2^-53 rounds to 1), then lane 16's (again 1);
    # adding the two small values first would give 1 + 2^-52
    v = np.zeros(64)
    v[0], v[32], v[16] = 1.0, 2.0**-53, 2.0**-53
    assert (pu.butterfly(v, "sum") == 1.0).all() and (2.0**-53 + 2.0**-53) + 1.0 == 1.0 + 2.0**-52
    # ... and lanes 1 and 33 would meet first under m = 32: 2^-53 + 2^-53 = 2^-52 survives
    v = np.zeros(64)
    v[0], v[1], v[33] = 1.0, 2.0**-53, 2.0**-53
    assert (pu.butterfly(v, "sum") == 1.0 + 2.0**-52).all()
    w = np.full(64, -INF)
    assert (pu.butterfly(w, "max") == -INF).all()
    w[17] = -3.0
    assert (pu.butterfly(w, "max") == -3.0).all()
    w[40] = NAN
    assert np.isnan(pu.butterfly(w, "max")).all()
    iv = np.full(64, 2**62, np.int64)
    assert (pu.butterfly(iv, "sum") == 0).all()   # 64 * 2^62 = 2^68 wraps to 0
    # two waves: block_sum adds the waves' sums from 0.0 in wave order, wave_sum keeps them apart
    x = np.zeros(128)
    x[0], x[64] = 1.0, 2.0**-53
    assert (pu.ref_block_reduce("block_sum", 128, x) == 1.0).all()
    assert pu.ref_block_reduce("wave_sum", 128, x).tolist() == [1.0] * 64 + [2.0**-53] * 64
    x[64] = 3.0
    assert (pu.ref_block_reduce("block_max", 128, x) == 3.0).all()
    assert pu.ref_block_reduce("wave_max", 128, x).tolist() == [1.0] * 64 + [3.0] * 64
    assert (pu.ref_block_reduce("block_max", 64, np.full(64, -INF)) == -INF).all()


def test_ref_block_owner_by_hand():
    assert pu.ref_block_owner([0, 0, 3, 3, 3, 10], 12).tolist() == [1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 5, 5]
    assert pu.ref_block_owner([0], 3).tolist() == [0, 0, 0]
