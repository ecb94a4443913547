// Device bodies that kernels of more than one PageRank unit instantiate, each defined here once:
// the kinds' set hash, insert and verify (mr_pr_kinds.hip's kernels and the batched set-up's
// k_kind_insert_b / k_kind_verify_b in mr_pr_setup.hip; kind_owner in mr_pr_shard.hip hashes with
// the same mix64) and the wave tiles' chunk scan (mr_pr_prepare.hip and the layout-order set-up).
// (mr_ingest.hip's mix64 is another function: it does not add the increment first.)
#pragma once
#include "mr_internal.h"
#include "mr_prim.h"

// (internal linkage, as every kernel of these units has: the bodies' __shared__ arrays are then
// private to the one kernel they are inlined into, which the compiler's alias analysis relies on)
namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr int KB = 256, KLDS = 512;   // kinds: block size, LDS table slots

// Set hash of a trace's key (its distinct ascending op ids, fp32(1/len_t), the id count):
// mix64(mix64(seed ^ wb ^ n << 32) + sum_op mix64(op ^ seed)).  Order-free, so the per-thread
// walk below and k_kind_insert's cooperative u16 form give the same key for the same trace (a
// requirement across ranks of a sharded graph).  CHK: a second, independently seeded hash of
// the same words, which travels with the key between ranks to catch a 64-bit key collision.
__device__ __forceinline__ uint64_t kind_fold(uint64_t seed, uint64_t wb, int64_t n, uint64_t acc) {
    const uint64_t h = mix64(mix64(seed ^ wb ^ ((uint64_t)n << 32)) + acc);
    return h ? h : 1;
}
template <bool CHK>
__device__ __forceinline__ uint64_t kind_hash2(const int64_t* off, const int32_t* ops, const float* w_t,
                                               int32_t t, uint64_t seed, uint64_t seed2, uint64_t* h2) {
    const int64_t e0 = off[t], e1 = off[t + 1];
    const uint64_t wb = e1 > e0 ? (uint64_t)__float_as_uint(w_t[t]) : 0ull;
    uint64_t a = 0, a2 = 0;
    for (int64_t e = e0; e < e1; ++e) {
        const uint64_t o = (uint64_t)(uint32_t)ops[e];
        a += mix64(o ^ seed);
        if (CHK) a2 += mix64(o ^ seed2);
    }
    if (CHK) *h2 = kind_fold(seed2, wb, e1 - e0, a2);
    return kind_fold(seed, wb, e1 - e0, a);
}
constexpr uint64_t KCHK_SEED = 0x0ddba11cafeull;

// Two-level insertion: traces of a block are first counted in an LDS table (hot kinds -- the
// same few call paths in thousands of traces -- would otherwise serialise on one global
// counter), then each distinct key of the block does ONE global insert + add.
// CHK (sharded graphs on >1 rank): the representative's check hash is stored per global slot
// (chk) for the cross-rank merge, computed in the same walk instead of a later re-read.
// IDW 2 / 4 (u16 ids, N <= 65536 / int32 ids): the block's 256 traces are hashed cooperatively --
// the threads stream the block's contiguous id range in aligned 16-B chunks (8 / 4 ids), coalesced
// across the wave, and add mix64(op) into per-trace LDS sums (an order-free SET hash: the ids of a
// trace are distinct and ascending, so the set is the list).  The walk-per-thread form (IDW 0,
// MR_KIND_WALK) reads one trace per lane, ~60 B apart (C5's kinds: 4.6 ms of dependent loads).
// Either hash only buckets traces; membership is decided by an exact comparison.
// Set hashes of the block's KB traces (tb = first trace), through per-trace LDS sums (loff, lacc,
// lacc2: KB + 1 / KB / KB entries) or a walk per thread.  Every thread of the block must call it;
// *h (and *h2 with CHK) is set for t < T.
// IDW (id width of the cooperative walk): 2 -- u16 ids (rs16, N <= 65536), 4 -- int32 ids (wide
// graphs: C5's 100k ops; the same 16-B chunks, 4 ids each), 0 -- a walk per thread (MR_KIND_WALK).
template <bool CHK, int IDW>
__device__ __forceinline__ void kind_block_hash(const int64_t* off, const int32_t* ops, const uint16_t* o16,
                                                const float* w_t, int32_t T, int32_t tb, uint64_t seed, int64_t* loff,
                                                unsigned long long* lacc, unsigned long long* lacc2, uint64_t* h,
                                                uint64_t* h2) {
    const int32_t t = tb + threadIdx.x;
    if constexpr (IDW != 0) {
        constexpr int IPC = IDW == 2 ? 8 : 4;   // ids per 16-B chunk
        __shared__ int64_t s_end;               // the id array's end (the last chunk's loads stop there)
        const int nt = min(KB, T - tb);
        if ((int)threadIdx.x < nt) {
            loff[threadIdx.x] = off[t];
            lacc[threadIdx.x] = 0ull;
            if (CHK) lacc2[threadIdx.x] = 0ull;
        }
        if (threadIdx.x == 0) {
            loff[nt] = off[tb + nt];
            s_end = off[T];
        }
        __syncthreads();
        const int64_t b = loff[0], e = loff[nt], eall = s_end;
        for (int64_t c = (b & ~(int64_t)(IPC - 1)) + (int64_t)IPC * threadIdx.x; c < e; c += (int64_t)IPC * KB) {
            uint32_t wd[4];
            if (IDW == 2 || c + IPC <= eall) {   // (rs16 holds nnz + 8 ids)
                const uint4 v = IDW == 2 ? *reinterpret_cast<const uint4*>(o16 + c)
                                         : *reinterpret_cast<const uint4*>(ops + c);
                wd[0] = v.x, wd[1] = v.y, wd[2] = v.z, wd[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) wd[k] = c + k < eall ? (uint32_t)ops[c + k] : 0u;
            }
            const int64_t p0 = c > b ? c : b;
            int lo = 0, hi = nt - 1;   // the trace holding p0: last lt with loff[lt] <= p0
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (loff[mid] <= p0) lo = mid;
                else hi = mid - 1;
            }
            int lt = lo;
            int64_t nb = loff[lt + 1];
            unsigned long long a = 0ull, a2 = 0ull;
            bool any = false;
#pragma unroll
            for (int k = 0; k < IPC; ++k) {
                const int64_t idx = c + k;
                if (idx < b || idx >= e) continue;
                while (idx >= nb) {
                    if (any) {
                        atomicAdd(&lacc[lt], a);
                        if (CHK) atomicAdd(&lacc2[lt], a2);
                    }
                    a = a2 = 0ull;
                    any = false;
                    ++lt;
                    nb = loff[lt + 1];
                }
                const uint64_t op = IDW == 2 ? (wd[k >> 1] >> ((k & 1) * 16)) & 0xffffu : (uint64_t)wd[k];
                a += mix64(op ^ seed);
                if (CHK) a2 += mix64(op ^ KCHK_SEED);
                any = true;
            }
            if (any) {
                atomicAdd(&lacc[lt], a);
                if (CHK) atomicAdd(&lacc2[lt], a2);
            }
        }
        __syncthreads();
    }
    if (t < T) {
        if constexpr (IDW != 0) {
            const int64_t n = loff[threadIdx.x + 1] - loff[threadIdx.x];
            const uint64_t wb = n > 0 ? (uint64_t)__float_as_uint(w_t[t]) : 0ull;
            *h = kind_fold(seed, wb, n, lacc[threadIdx.x]);
            if (CHK) *h2 = kind_fold(KCHK_SEED, wb, n, lacc2[threadIdx.x]);
        } else {
            *h = kind_hash2<CHK>(off, ops, w_t, t, seed, KCHK_SEED, h2);
        }
    }
}

template <bool CHK, int IDW>
__device__ __forceinline__ void kind_insert_body(int32_t blk, const int64_t* off, const int32_t* ops, const uint16_t* o16,
                                                 const float* w_t, int32_t T, unsigned long long* hk, KCnt* cr,
                                                 int32_t* slot_of, uint64_t mask, uint64_t seed, uint64_t* chk,
                                                 uint64_t hmask) {
    __shared__ unsigned long long lkey[KLDS];
    __shared__ uint32_t lcnt[KLDS];
    __shared__ int32_t lrep[KLDS];
    __shared__ int32_t lglob[KLDS];
    __shared__ uint64_t lchk[CHK ? KLDS : 1];
    __shared__ int64_t loff[IDW ? KB + 1 : 1];
    __shared__ unsigned long long lacc[IDW ? KB : 1], lacc2[IDW && CHK ? KB : 1];
    for (int i = threadIdx.x; i < KLDS; i += KB) {
        lkey[i] = 0ull;
        lcnt[i] = 0u;
        lrep[i] = 0x7fffffff;
    }
    const int32_t tb = blk * KB;
    const int32_t t = tb + threadIdx.x;
    uint64_t h = 0, h2 = 0;
    kind_block_hash<CHK, IDW>(off, ops, o16, w_t, T, tb, seed, loff, lacc, lacc2, &h, &h2);
    __syncthreads();
    int myslot = -1;
    if (t < T) {
        h &= hmask;   // ~0 (tests narrow it to force collisions)
        if (!h) h = 1;
        int s = (int)(h & (KLDS - 1));
        for (;;) {
            unsigned long long k = atomicCAS(&lkey[s], 0ull, (unsigned long long)h);
            if (k == 0ull || k == h) break;
            s = (s + 1) & (KLDS - 1);
        }
        atomicAdd(&lcnt[s], 1u);
        atomicMin(&lrep[s], t);   // the class's lowest trace of the block (deterministic)
        myslot = s;
    }
    __syncthreads();
    if (CHK && myslot >= 0 && lrep[myslot] == t) lchk[myslot] = h2;
    __syncthreads();
    for (int i = threadIdx.x; i < KLDS; i += KB) {
        const uint64_t h = lkey[i];
        if (!h) continue;
        uint64_t slot = h & mask;
        for (;;) {
            const uint64_t k = atomicCAS(&hk[slot], 0ull, (unsigned long long)h);
            if (k == 0 || k == h) {   // the representative: the class's lowest trace over the blocks
                atomicMin(&cr[slot].rep, lrep[i]);   // (read after this kernel; deterministic)
                if (k == 0 && CHK) chk[slot] = lchk[i];
                break;
            }
            slot = (slot + 1) & mask;
        }
        atomicAdd(&cr[slot].cnt, lcnt[i]);
        lglob[i] = (int32_t)slot;
    }
    __syncthreads();
    if (t < T) slot_of[t] = lglob[myslot];
}

template <typename ID>   // int32 ids, or their u16 copy (rs16)
__device__ __forceinline__ void kind_verify_body(int32_t t, const int64_t* off, const ID* ops, const float* w_t, int32_t T,
                                                 const KCnt* cr, const int32_t* slot_of, double* kind, int32_t* flag,
                                                 int32_t* krep) {
    if (t >= T) return;
    const KCnt ks = cr[slot_of[t]];
    const int32_t r = ks.rep;
    kind[t] = (double)ks.cnt;
    if (krep) krep[t] = r;   // (kind compression: the class representative)
    if (r == t) return;
    int64_t a0 = off[t], a1 = off[t + 1], b0 = off[r], b1 = off[r + 1];
    bool eq = (a1 - a0) == (b1 - b0);
    if (eq && a1 > a0) eq = __float_as_uint(w_t[t]) == __float_as_uint(w_t[r]);
    for (int64_t i = 0; eq && i < a1 - a0; ++i) eq = ops[a0 + i] == ops[b0 + i];
    if (!eq) atomicOr(flag, 1);
}

// chunks of 4 ids per wave tile (its last position holds its longest trace: lengths ascend), their
// exclusive prefix and its int32 copy in one launch: runs of TS_TILE wave tiles per block, chained
// by decoupled look-back
constexpr int TS_T = 256, TS_I = 8, TS_TILE = TS_T * TS_I;
__device__ __forceinline__ void tr_chunk_scan_body(int32_t tile_, int32_t ntiles, const int32_t* tperm,
                                                   const int64_t* off, int32_t T, int32_t n_wt, int64_t* c64,
                                                   int32_t* coff, unsigned long long* st, uint64_t epoch) {
    __shared__ int64_t sa[TS_T];
    __shared__ int64_t ex;
    const int tid = threadIdx.x;
    const int64_t tile = tile_, base = tile * TS_TILE + (int64_t)tid * TS_I;
    int64_t v[TS_I], a = 0;
#pragma unroll
    for (int i = 0; i < TS_I; ++i) {
        const int64_t k = base + i;
        v[i] = 0;
        if (k < n_wt) {
            const int32_t t = tperm[min(k * WAVE + WAVE - 1, (int64_t)T - 1)];
            v[i] = (off[t + 1] - off[t] + 3) >> 2;
        }
        a += v[i];
    }
    sa[tid] = a;
    __syncthreads();
    for (int o = 1; o < TS_T; o <<= 1) {
        const int64_t x = tid >= o ? sa[tid - o] : 0;
        __syncthreads();
        sa[tid] += x;
        __syncthreads();
    }
    if (tid < WAVE) {
        const int64_t e = dl_lookback_wave(st, tile, sa[TS_T - 1], epoch);
        if (tid == 0) ex = e;
        if (tid == 0 && tile == (int64_t)ntiles - 1) {
            c64[n_wt] = ex + sa[TS_T - 1];
            coff[n_wt] = (int32_t)(ex + sa[TS_T - 1]);
        }
    }
    __syncthreads();
    int64_t r = ex + sa[tid] - a;
#pragma unroll
    for (int i = 0; i < TS_I; ++i) {
        const int64_t k = base + i;
        if (k < n_wt) {
            c64[k] = r;
            coff[k] = (int32_t)r;
        }
        r += v[i];
    }
}

}  // namespace
