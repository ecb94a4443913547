"""ctypes loader of the test-only library (tests/csrc/mr_selftest.hip -> microrank_amd/libmicrorank_selftest.so)
and the plain references of the device primitives it drives: numpy and Python integers only.

The references are checked on hand-computed cases in test_primitives_surface.py, so that a wrong
reference cannot agree with a wrong kernel."""
import ctypes as C
import os

import numpy as np

from microrank_amd import _lib

SELFTEST_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libmicrorank_selftest.so")

P = C.c_void_p
# name -> (restype, argtypes): every entry point of mr_selftest.hip
SIGNATURES = {
    "mrt_scan": (C.c_int, [P, P, C.c_int, C.c_int64, C.c_int, P]),
    "mrt_set_scan_epoch": (C.c_int, [P, C.c_uint32]),
    "mrt_scan_state": (C.c_int, [P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "mrt_sort": (C.c_int, [P, P, P, C.c_int64, C.c_int]),
    "mrt_bits_for": (C.c_int, [C.c_uint64]),
    "mrt_runs": (C.c_int, [P, C.c_int, P, P, P, C.c_int64, P, P, P, P]),
    "mrt_evtable": (C.c_int, [P, C.c_int, C.c_int, P, P, C.c_int64, C.c_int64, C.c_int, C.c_int, P]),
    "mrt_block_reduce": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int64, P]),
    "mrt_block_owner": (C.c_int, [P, P, C.c_int32, C.c_int32, P]),
}

# constants of mr_prim.hip / mr_sort.hip / mr_prim.h / mr_evidence.h that the cases aim at
WAVE = 64
SCAN_SINGLE_MAX = 16384   # one-block scan up to here
SCAN_TILE = 2048          # look-back tile
SCAN_WORDS_MIN = 8192     # status words of a context's first look-back scan
DL_EB, DL_VB = 20, 42     # epoch and value bits of a status word
SORT_LDS_MAX = 4096       # bitonic sort in LDS up to here
SORT_TILE = 2048          # radix tile
EV_HB = 10
EV_H = 1 << EV_HB
EV_BIAS = 1 << 63
M64 = (1 << 64) - 1
OPS = {"block_sum": 0, "block_max": 1, "wave_sum": 2, "wave_max": 3, "wave_sum_i64": 4}

_st = None


def load():
    """The selftest library (the product library first: one mapping serves both)."""
    global _st
    if _st is None:
        _lib.load()
        lib = C.CDLL(SELFTEST_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _st = lib
    return _st


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


# ---------------------------------------------------------------- device calls
def scan(ctx, a, in_place=False):
    """Exclusive scan of int64 or int32 counts: n + 1 int64 offsets."""
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.int64, np.int32)
    out = np.full(a.size + 1, -1, np.int64)
    ctx.check(load().mrt_scan(ctx.h, _p(a), int(a.dtype == np.int32), a.size, int(in_place), _p(out)), "mrt_scan")
    return out


def set_scan_epoch(ctx, epoch):
    ctx.check(load().mrt_set_scan_epoch(ctx.h, epoch), "mrt_set_scan_epoch")


def scan_state(ctx):
    """(epoch of the last look-back scan, status words the context holds)"""
    e, w = C.c_uint32(0), C.c_uint64(0)
    ctx.check(load().mrt_scan_state(ctx.h, C.byref(e), C.byref(w)), "mrt_scan_state")
    return e.value, w.value


def sort(ctx, keys, vals, bits):
    """Copies of keys (and vals, or None) sorted on the keys' low `bits` bits."""
    k = _arr(keys, np.uint64).copy()
    v = None if vals is None else _arr(vals, np.uint32).copy()
    ctx.check(load().mrt_sort(ctx.h, _p(k), _p(v), k.size, bits), "mrt_sort")
    return k, v


def bits_for(v):
    return load().mrt_bits_for(v)


def runs(ctx, key_bits, keys, has, d):
    """Per lane of the stream cut into 64-lane waves: (n, sum, biased max, is-last)."""
    keys, has, d = _arr(keys, np.int64), _arr(has, np.uint8), _arr(d, np.uint64)
    n = keys.size
    on, os_, om, ol = np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint8)
    ctx.check(load().mrt_runs(ctx.h, key_bits, _p(keys), _p(has), _p(d), n, _p(on), _p(os_), _p(om), _p(ol)), "mrt_runs")
    return on, os_, om, ol


def evtable(ctx, key_bits, direct, keys, d, n_keys, blocks, tiles):
    """The dense counters [n_keys, 3] (n, sum, biased max) after one launch of blocks x tiles x 256 rows."""
    keys, d = _arr(keys, np.int64), _arr(d, np.uint64)
    cnt = np.empty((n_keys, 3), np.uint64)
    ctx.check(load().mrt_evtable(ctx.h, key_bits, int(direct), _p(keys), _p(d), keys.size, n_keys, blocks, tiles, _p(cnt)),
              "mrt_evtable")
    return cnt


def block_reduce(ctx, op, block, v):
    """What every thread holds after OPS[op] over blocks of `block` threads (v.size a multiple of it)."""
    v = np.ascontiguousarray(v)
    assert v.dtype == (np.int64 if op == "wave_sum_i64" else np.float64)
    out = np.empty_like(v)
    ctx.check(load().mrt_block_reduce(ctx.h, OPS[op], block, _p(v), v.size, _p(out)), "mrt_block_reduce")
    return out


def block_owner(ctx, first, n_blocks):
    first = _arr(first, np.int32)
    out = np.empty(n_blocks, np.int32)
    ctx.check(load().mrt_block_owner(ctx.h, _p(first), first.size, n_blocks, _p(out)), "mrt_block_owner")
    return out


# ---------------------------------------------------------------- references
def ref_scan(a):
    out = np.zeros(a.size + 1, np.int64)
    np.cumsum(a, dtype=np.int64, out=out[1:])
    return out


def ref_sort_perm(keys, bits):
    mask = np.uint64(M64 if bits >= 64 else (1 << bits) - 1)
    return np.argsort(_arr(keys, np.uint64) & mask, kind="stable")


def ref_runs(keys, has, d):
    """The stream in waves of 64 lanes (the last one filled with key -1, no value); inside a wave, runs of
    adjacent equal keys.  Per lane, over its run up to and including the lane: how many lanes brought a
    value, their sum mod 2^64, the largest d ^ 2^63 among them (0: none); and whether the lane ends its run."""
    keys = [int(k) for k in keys]
    has = [bool(h) for h in has]
    d = [int(x) for x in d]
    n = len(keys)
    pad = -n % WAVE
    keys, has, d = keys + [-1] * pad, has + [False] * pad, d + [0] * pad
    on, os_, om, ol = [], [], [], []
    for w0 in range(0, len(keys), WAVE):
        cn = cs = cm = 0
        for l in range(WAVE):
            i = w0 + l
            if l == 0 or keys[i] != keys[i - 1]:
                cn = cs = cm = 0
            if has[i]:
                cn += 1
                cs = (cs + d[i]) & M64
                cm = max(cm, d[i] ^ EV_BIAS)
            on.append(cn)
            os_.append(cs)
            om.append(cm)
            ol.append(int(l == WAVE - 1 or keys[i + 1] != keys[i]))
    return (np.array(on[:n], np.uint64), np.array(os_[:n], np.uint64), np.array(om[:n], np.uint64),
            np.array(ol[:n], np.uint8))


def ev_hash(k):
    """EvTable's slot of key k in hashed mode (mr_evidence.h: the top EV_HB bits of k * 0x9E3779B97F4A7C15)."""
    return ((int(k) * 0x9E3779B97F4A7C15) & M64) >> (64 - EV_HB)


def ref_evtable(keys, d, n_keys):
    keys, d = _arr(keys, np.int64), _arr(d, np.uint64)
    live = keys >= 0
    k, v = keys[live], d[live]
    cnt = np.zeros((n_keys, 3), np.uint64)
    np.add.at(cnt[:, 0], k, np.uint64(1))
    np.add.at(cnt[:, 1], k, v)   # (uint64: wraps mod 2^64)
    np.maximum.at(cnt[:, 2], k, v ^ np.uint64(EV_BIAS))
    return cnt


def _nmax(a, b):
    """mr_prim.h nmax, elementwise: a NaN on either side wins, else the larger."""
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(a > b, a, b)))


def butterfly(v, op):
    """A wave's xor butterfly over its 64 values, m = 32, 16, ..., 1: what every lane holds after each
    lane combined its value with lane ^ m's ("sum": +, "max": nmax).  Returns all 64 lanes."""
    v = np.array(v, copy=True)
    assert v.size == WAVE
    idx = np.arange(WAVE)
    m = 32
    while m >= 1:
        o = v[idx ^ m]
        with np.errstate(over="ignore", invalid="ignore"):
            v = v + o if op == "sum" else _nmax(v, o)
        m >>= 1
    return v


def ref_block_reduce(op, block, v):
    """What every thread holds: the waves' butterflies, then (block_*) the waves combined serially from
    0.0 / -inf in wave order."""
    v = np.ascontiguousarray(v)
    out = np.empty_like(v)
    kind = "max" if op.endswith("max") else "sum"
    with np.errstate(over="ignore", invalid="ignore"):
        for b0 in range(0, v.size, block):
            waves = [butterfly(v[w0:w0 + WAVE], kind) for w0 in range(b0, b0 + block, WAVE)]
            if op.startswith("wave"):
                out[b0:b0 + block] = np.concatenate(waves)
                continue
            t = np.float64(0.0 if kind == "sum" else -np.inf)
            for w in waves:
                t = t + w[0] if kind == "sum" else _nmax(t, w[0])
            out[b0:b0 + block] = t
    return out


def ref_block_owner(first, n_blocks):
    return (np.searchsorted(_arr(first, np.int64), np.arange(n_blocks), side="right") - 1).astype(np.int32)
