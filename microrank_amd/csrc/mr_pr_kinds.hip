// Kinds for K2 (pagerank.py:54-66), and the kind-compressed graph built from them.
// kind[t] = size of the class of traces with an equal P_sr column: key = (op set, fp32(1/len_t)).
// Open-addressing hash table of 64-bit keys; a second pass verifies every member against the
// slot's representative, so a hash collision is detected (flag) rather than miscounted.
// (the set hash and the insert / verify bodies, which the batched set-up instantiates too: mr_pr_dev.h)
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "mr_pr_dev.h"
#include "mr_pr_internal.h"
#include "mr_sort.h"

namespace {

template <bool CHK, int IDW>
__global__ void __launch_bounds__(KB) k_kind_insert(const int64_t* off, const int32_t* ops, const uint16_t* o16,
                                                    const float* w_t, int32_t T, unsigned long long* hk, KCnt* cr, int32_t* slot_of,
                                                    uint64_t mask, uint64_t seed, uint64_t* chk, uint64_t hmask) {
    kind_insert_body<CHK, IDW>((int32_t)blockIdx.x, off, ops, o16, w_t, T, hk, cr, slot_of, mask, seed, chk, hmask);
}

template <typename ID>
__global__ void k_kind_verify(const int64_t* off, const ID* ops, const float* w_t, int32_t T,
                              const KCnt* cr, const int32_t* slot_of, double* kind, int32_t* flag, int32_t* krep) {
    kind_verify_body<ID>((int32_t)(blockIdx.x * blockDim.x + threadIdx.x), off, ops, w_t, T, cr, slot_of, kind, flag, krep);
}

// Kinds by partition (graphs on one rank), no global hash table:
//   k_kind_rec     per block of KB traces: set hashes, equal keys merged in an LDS table into
//                  RECORDS (key, count, first trace) -- a hot kind (thousands of traces on one
//                  call path) leaves one record per block, so no later atomic serialises on it --
//                  and the records counted per partition (the key's top bits);
//   k_kind_rscatter a counting sort of the records into partitions of ~KP_MEAN;
//   k_kind_part    a block per partition merges its records in an LDS table (count sum, first
//                  trace min): every record then holds its class's size and representative;
//   k_kind_final   per trace: kind = its record's class size; every member is checked against
//                  the representative (ops and fp32(1/len_t), exactly): a hash collision raises
//                  flag word 0 (retry with the next seed), never a miscount.
// graphs of at least this many traces take the partition path (below: the LDS-aggregated global
// table).  1M measured ahead of 2M for C4's rank-0-of-8 share (1.25M traces: step 1.50 -> 1.44 ms,
// profiles/r05/r05r_kind_part_ab.txt); MR_KIND_PART_MIN overrides (read per call)
constexpr int64_t KIND_PART_MIN_DEFAULT = (int64_t)1 << 20;
constexpr int KP_MEAN = 1024;   // mean records per partition (at most)
constexpr int KP_LDS = 4096;    // LDS table slots of a partition block
constexpr int KP_B = 256;
__device__ __forceinline__ int32_t kind_part(uint64_t h, int pb) { return pb ? (int32_t)(h >> (64 - pb)) : 0; }
// a record: key, count, first trace -- one 16-B store / load where three arrays cost three
// scattered partial-line writes per record in k_kind_rscatter
struct __attribute__((aligned(16))) KRec {
    unsigned long long h;
    uint32_t c;
    int32_t r;
};
template <int IDW>
__global__ void __launch_bounds__(KB) k_kind_rec(const int64_t* off, const int32_t* ops, const uint16_t* o16,
                                                 const float* w_t, int32_t T, uint64_t seed, uint64_t hmask, int pb,
                                                 KRec* rec_out, int32_t* nrec, int32_t* rec_of, int32_t* hist) {
    __shared__ unsigned long long lkey[KLDS];
    __shared__ uint32_t lcnt[KLDS];
    __shared__ int32_t lrep[KLDS];
    __shared__ int32_t lidx[KLDS];
    __shared__ int32_t ln;
    __shared__ int64_t loff[IDW ? KB + 1 : 1];
    __shared__ unsigned long long lacc[IDW ? KB : 1], lacc2[1];
    for (int i = threadIdx.x; i < KLDS; i += KB) {
        lkey[i] = 0ull;
        lcnt[i] = 0u;
        lrep[i] = 0x7fffffff;
    }
    if (threadIdx.x == 0) ln = 0;
    const int32_t tb = blockIdx.x * KB, t = tb + threadIdx.x;
    uint64_t h = 0, h2 = 0;
    kind_block_hash<false, IDW>(off, ops, o16, w_t, T, tb, seed, loff, lacc, lacc2, &h, &h2);
    __syncthreads();
    int s = -1;
    if (t < T) {
        h &= hmask;   // ~0 (tests narrow it to force collisions)
        if (!h) h = 1;
        s = (int)(h & (KLDS - 1));
        for (;;) {   // <= KB distinct keys in KLDS = 2 KB slots: always a free slot
            const unsigned long long k = atomicCAS(&lkey[s], 0ull, (unsigned long long)h);
            if (k == 0ull || k == h) break;
            s = (s + 1) & (KLDS - 1);
        }
        atomicAdd(&lcnt[s], 1u);
        atomicMin(&lrep[s], t);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KLDS; i += KB) {
        const uint64_t k = lkey[i];
        if (!k) continue;
        const int32_t r = atomicAdd(&ln, 1);   // record order within the block: free (sums / mins)
        lidx[i] = r;
        KRec v;
        v.h = k;
        v.c = lcnt[i];
        v.r = lrep[i];
        rec_out[(int64_t)tb + r] = v;
        if (hist) atomicAdd(&hist[kind_part(k, pb)], 1);   // (the cursor scatter's counts)
    }
    __syncthreads();
    if (t < T) rec_of[t] = tb + lidx[s];
    if (threadIdx.x == 0) nrec[blockIdx.x] = ln;
}
__global__ void k_kind_rscatter(const KRec* rin, const int32_t* nrec, int32_t T, int pb, unsigned long long* cur,
                                KRec* e, int32_t* rpos) {
    const int32_t rec = blockIdx.x * blockDim.x + threadIdx.x;
    if (rec >= T || (rec % KB) >= nrec[rec / KB]) return;
    const KRec v = rin[rec];
    const int32_t pos = (int32_t)atomicAdd(&cur[kind_part(v.h, pb)], 1ull);
    e[pos] = v;
    rpos[rec] = pos;
}
// The records grouped by partition in two passes over the partition's bits, with no device atomic
// per record (the cursor scatter above takes two: its counts and its cursor, 7.4 ms of C5's
// 100M records):
//   k_kp1_count   tiles of KT slots: per tile a histogram of the partition's top b1 bits (the
//                 coarse bucket), written bucket-major (cnt[b * ntile + tile]), so ONE exclusive
//                 scan of it gives every (bucket, tile)'s first position;
//   k_kp1_scatter the tile's records to their buckets through LDS cursors, each with its slot;
//   k_kp2         a block per bucket: counts its fine partitions (the next pb - b1 bits) in LDS,
//                 writes their starts, and scatters the bucket's records into partition order
//                 inside the bucket's range, each beside its block-order slot (eslot).
// The order inside a partition depends on LDS atomics; k_kind_part's merge (sums, minimum) does
// not: the same classes and representatives.
constexpr int KP1_B = 8;    // coarse bits (1024 buckets over tiles of 16384 measured slower at C4: 584 vs 553 us)
constexpr int KT = 4096;    // slots per level-1 tile
constexpr int KT_T = 256;   // threads of a level-1 block
constexpr int KP2_T = 1024;
__device__ __forceinline__ int32_t kbits(uint64_t h, int n) { return n ? (int32_t)(h >> (64 - n)) : 0; }
// (the three loops take KP_BATCH records per thread per round: loads first, then the LDS atomics
// and stores -- one round's loads in flight together instead of one dependent chain per record)
constexpr int KP_BATCH = 4;
__global__ void __launch_bounds__(KT_T) k_kp1_count(const KRec* __restrict__ rec, const int32_t* __restrict__ nrec,
                                                    int64_t R, int b1, int32_t ntile, int32_t* __restrict__ cnt) {
    __shared__ int32_t hb[1 << KP1_B];
    const int nbk = 1 << b1;
    for (int i = threadIdx.x; i < nbk; i += KT_T) hb[i] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * KT;
    for (int k0 = 0; k0 < KT / KT_T; k0 += KP_BATCH) {
        int bk[KP_BATCH];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            const int64_t sl = s0 + (k0 + j) * KT_T + threadIdx.x;
            bk[j] = sl < R && (int32_t)(sl % KB) < nrec[sl / KB] ? kbits(rec[sl].h, b1) : -1;
        }
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j)
            if (bk[j] >= 0) atomicAdd(&hb[bk[j]], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nbk; i += KT_T) cnt[(int64_t)i * ntile + blockIdx.x] = hb[i];
}
__global__ void __launch_bounds__(KT_T) k_kp1_scatter(const KRec* __restrict__ rec, const int32_t* __restrict__ nrec,
                                                      int64_t R, int b1, int32_t ntile, const int64_t* __restrict__ off,
                                                      KRec* __restrict__ out, uint32_t* __restrict__ oslot) {
    __shared__ int64_t base[1 << KP1_B];   // the (bucket, tile)'s first position, and 32-bit cursors after it
    __shared__ uint32_t cur[1 << KP1_B];
    const int nbk = 1 << b1;
    for (int i = threadIdx.x; i < nbk; i += KT_T) {
        base[i] = off[(int64_t)i * ntile + blockIdx.x];
        cur[i] = 0u;
    }
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * KT;
    for (int k0 = 0; k0 < KT / KT_T; k0 += KP_BATCH) {
        KRec v[KP_BATCH];
        bool ok[KP_BATCH];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            const int64_t sl = s0 + (k0 + j) * KT_T + threadIdx.x;
            ok[j] = sl < R && (int32_t)(sl % KB) < nrec[sl / KB];
            if (ok[j]) v[j] = rec[sl];
        }
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            if (!ok[j]) continue;
            const int b = kbits(v[j].h, b1);
            const int64_t pos = base[b] + (int64_t)atomicAdd(&cur[b], 1u);
            out[pos] = v[j];
            oslot[pos] = (uint32_t)(s0 + (k0 + j) * KT_T + threadIdx.x);
        }
    }
}
__global__ void __launch_bounds__(KP2_T) k_kp2(const KRec* __restrict__ in, const uint32_t* __restrict__ islot,
                                               const int64_t* __restrict__ off, int pb, int b1, int32_t ntile,
                                               KRec* __restrict__ out, uint32_t* __restrict__ eslot,
                                               int64_t* __restrict__ pstart) {
    extern __shared__ int64_t kp2[];   // [KP2_T] scan partials, then [nf] 32-bit counts / cursors (from B0)
    const int nf = 1 << (pb - b1), b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t B0 = off[(int64_t)b * ntile], B1 = off[(int64_t)(b + 1) * ntile];
    int64_t* part = kp2;
    uint32_t* cur = (uint32_t*)(kp2 + KP2_T);
    for (int f = tid; f < nf; f += KP2_T) cur[f] = 0u;
    __syncthreads();
    const uint64_t fm = (uint64_t)nf - 1;
    for (int64_t i0 = B0 + tid; i0 < B1; i0 += (int64_t)KP2_T * KP_BATCH) {
        int fk[KP_BATCH];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            const int64_t i = i0 + (int64_t)j * KP2_T;
            fk[j] = i < B1 ? (int)((uint64_t)kbits(in[i].h, pb) & fm) : -1;
        }
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j)
            if (fk[j] >= 0) atomicAdd(&cur[fk[j]], 1u);
    }
    __syncthreads();
    // exclusive scan of the nf counts: a run of consecutive counts per thread, then its partials
    const int per = (nf + KP2_T - 1) / KP2_T, f0 = tid * per, f1 = min(f0 + per, nf);
    int64_t a = 0;
    for (int f = f0; f < f1; ++f) a += cur[f];
    part[tid] = a;
    __syncthreads();
    for (int o = 1; o < KP2_T; o <<= 1) {
        const int64_t x = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    int64_t run = part[tid] - a;   // (relative to B0)
    for (int f = f0; f < f1; ++f) {
        const uint32_t c = cur[f];
        cur[f] = (uint32_t)run;
        pstart[(int64_t)b * nf + f] = B0 + run;
        run += c;
    }
    if (b == (int)gridDim.x - 1 && tid == 0) pstart[(int64_t)gridDim.x * nf] = B1;
    __syncthreads();
    for (int64_t i0 = B0 + tid; i0 < B1; i0 += (int64_t)KP2_T * KP_BATCH) {
        KRec v[KP_BATCH];
        uint32_t sl[KP_BATCH];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            const int64_t i = i0 + (int64_t)j * KP2_T;
            if (i < B1) {
                v[j] = in[i];
                sl[j] = islot[i];
            }
        }
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            if (i0 + (int64_t)j * KP2_T >= B1) continue;
            const int64_t pos = B0 + (int64_t)atomicAdd(&cur[(uint64_t)kbits(v[j].h, pb) & fm], 1u);
            out[pos] = v[j];
            eslot[pos] = sl[j];   // (beside the record, in partition order: k_kind_part writes back through it)
        }
    }
}
// eslot (two-pass grouping): each record's slot in the block-order records `back`, where the class
// (count, first trace) is written -- k_kind_final then reads it at rec_of[t] (a block's own range)
// instead of through a per-record position (a random read per trace); null: into e itself
__global__ void __launch_bounds__(KP_B) k_kind_part(const int64_t* pstart, KRec* e, int32_t* flag,
                                                    const uint32_t* eslot, KRec* back) {
    __shared__ unsigned long long tkey[KP_LDS];
    __shared__ uint32_t tcnt[KP_LDS];
    __shared__ int32_t trep[KP_LDS];
    const int64_t b = pstart[blockIdx.x], en = pstart[blockIdx.x + 1];
    for (int i = threadIdx.x; i < KP_LDS; i += KP_B) {
        tkey[i] = 0ull;
        tcnt[i] = 0u;
        trep[i] = 0x7fffffff;
    }
    __syncthreads();
    // (KP_BATCH records per thread per round: their loads go out together)
    for (int64_t i0 = b + threadIdx.x; i0 < en; i0 += (int64_t)KP_B * KP_BATCH) {
        KRec vv[KP_BATCH];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j)
            if (i0 + (int64_t)j * KP_B < en) vv[j] = e[i0 + (int64_t)j * KP_B];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            if (i0 + (int64_t)j * KP_B >= en) continue;
            const KRec& v = vv[j];
            const uint64_t h = v.h;
            int s = (int)(h & (KP_LDS - 1));
            for (int probe = 0;; ++probe) {
                if (probe == KP_LDS) {   // more distinct keys than slots: not with hashed partitions
                    atomicOr(flag + 2, 1);
                    break;
                }
                const unsigned long long k = atomicCAS(&tkey[s], 0ull, (unsigned long long)h);
                if (k == 0ull || k == h) {
                    atomicAdd(&tcnt[s], v.c);
                    atomicMin(&trep[s], v.r);   // the class's first trace (deterministic)
                    break;
                }
                s = (s + 1) & (KP_LDS - 1);
            }
        }
    }
    __syncthreads();
    for (int64_t i0 = b + threadIdx.x; i0 < en; i0 += (int64_t)KP_B * KP_BATCH) {
        uint64_t hh[KP_BATCH];
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) hh[j] = i0 + (int64_t)j * KP_B < en ? e[i0 + (int64_t)j * KP_B].h : 0ull;
#pragma unroll
        for (int j = 0; j < KP_BATCH; ++j) {
            const int64_t i = i0 + (int64_t)j * KP_B;
            if (i >= en) continue;
            const uint64_t h = hh[j];
            int s = (int)(h & (KP_LDS - 1));
            for (int probe = 0; probe < KP_LDS && tkey[s] != h; ++probe) s = (s + 1) & (KP_LDS - 1);
            if (tkey[s] != h) continue;   // (overflowed: flagged above)
            *(uint2*)&(eslot ? back[eslot[i]] : e[i]).c = make_uint2(tcnt[s], (uint32_t)trep[s]);   // (c, r): one 8-B store
        }
    }
}
template <typename ID>
__global__ void k_kind_final(const int32_t* rec_of, const int32_t* rpos, const KRec* e, const int64_t* off,
                             const ID* ops, const float* w_t, int32_t T, double* kind, int32_t* flag, int32_t* krep) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int32_t pos = rpos ? rpos[rec_of[t]] : rec_of[t];   // (null: e holds the classes in slot order)
    const uint2 cr = *(const uint2*)&e[pos].c;
    kind[t] = (double)cr.x;
    const int32_t r = (int32_t)cr.y;
    if (krep) krep[t] = r;   // (kind compression: the class representative)
    if (r == t) return;
    // exact membership: same ids and the same fp32(1/len_t) as the representative
    const int64_t a0 = off[t], a1 = off[t + 1], b0 = off[r], b1 = off[r + 1];
    bool eq = (a1 - a0) == (b1 - b0);
    if (eq && a1 > a0) eq = __float_as_uint(w_t[t]) == __float_as_uint(w_t[r]);
    for (int64_t j = 0; eq && j < a1 - a0; ++j) eq = ops[a0 + j] == ops[b0 + j];
    if (!eq) atomicOr(flag, 1);
}

// ---------------------------------------------------------------- kind compression (§8(f) f4)
// Traces of one kind have identical r (same op set and len_t, hence the same v_t): the iteration
// runs over one representative per kind whose q carries the kind's multiplicity.
__global__ void k_kc_flags(const int32_t* krep, int32_t T, int32_t* flag) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) flag[t] = krep[t] == t ? 1 : 0;
}
__global__ void k_kc_reps(const int32_t* flag, const int64_t* pos, int32_t T, const int64_t* off, const int32_t* len_t,
                          const double* kind, int32_t* rep, int32_t* len_c, double* mult, int32_t* cnt) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T || !flag[t]) return;
    const int64_t k = pos[t];
    rep[k] = t;
    len_c[k] = len_t[t];
    mult[k] = kind[t];
    cnt[k] = (int32_t)(off[t + 1] - off[t]);
}
__global__ void k_kc_ops(const int32_t* rep, const int64_t* off_c, int32_t K, const int64_t* off, const int32_t* ops,
                         int32_t* ops_c) {
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int32_t t = rep[k];
    const int64_t a = off[t], n = off[t + 1] - a, b = off_c[k];
    for (int64_t j = 0; j < n; ++j) ops_c[b + j] = ops[a + j];
}
__global__ void k_kc_mw(const int32_t* tperm, const float* w_tp, const double* mult, int32_t T, double* mw_tp) {
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < T) mw_tp[p] = (double)w_tp[p] * mult[tperm[p]];   // exact: a 24-bit mantissa times an integer < 2^29
}
__global__ void k_kc_tile_mult(const int32_t* tperm, const double* mult, int32_t T, int32_t n_wt, int64_t* out) {
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_wt) return;
    int64_t m = 0;
    for (int32_t p = k * WAVE; p < min(k * WAVE + WAVE, T); ++p) m += (int64_t)mult[tperm[p]];
    out[k] = m;
}

}  // namespace

// A 64-bit set-hash collision between two different trace kinds is caught by the exact
// verification; the whole call then reruns with the next seed (independent hash functions), so
// an input that collides under one seed is still ranked.  Seeds are a fixed sequence: every rank
// of a sharded graph takes the same one.
uint64_t kind_seed(int a) {
    static const uint64_t seed0 = [] {   // MR_KIND_SEED: test knob (start the sequence elsewhere)
        const char* e = getenv("MR_KIND_SEED");
        return e ? (uint64_t)strtoull(e, nullptr, 0) : 0x5eed5eedull;
    }();
    return seed0 + 0x9E3779B97F4A7C15ull * (uint64_t)a;
}
// MR_KIND_TEST_COLLIDE: test knob -- the first attempt keeps 2 bits of every key, so distinct
// kinds collide and the verification + retry path runs
uint64_t kind_hmask(int a) { return (a == 0 && getenv("MR_KIND_TEST_COLLIDE") != nullptr) ? 3ull : ~0ull; }
// traces from which the kinds take the partition path; MR_KIND_PART_MIN: test knob (read per call)
int64_t kind_part_min() {
    const char* kpe = getenv("MR_KIND_PART_MIN");
    return kpe ? (int64_t)atoll(kpe) : KIND_PART_MIN_DEFAULT;
}

// Kinds of g (pagerank.py:54-66) into g->kind, the class representative of each trace into
// g->krep when that is allocated; a 64-bit key collision sets flag word 0.
int graph_kinds(mr_ctx* ctx, mr_graph* g, bool chk, bool ktab, uint64_t cap, uint64_t seed, uint64_t hmask) {
    hipStream_t st = ctx->stream;
    const int32_t T = g->T;
    const int64_t* koff = g->rs_is_sr ? g->rs_off.p : g->srt_off.p;
    const int32_t* kops = g->rs_is_sr ? g->rs_ops.p : g->srt_ops.p;
    static const bool walk = getenv("MR_KIND_WALK") != nullptr;   // A/B knob: per-thread int32 walk
    const bool u16 = !walk && g->rs_is_sr && g->rs16.p != nullptr;   // rs16 = u16 copy of rs_ops
    if (ktab) {
        if (chk) MR_TRY(g->ht_chk.alloc(ctx, cap));
        auto kins = chk ? (u16 ? k_kind_insert<true, 2> : walk ? k_kind_insert<true, 0> : k_kind_insert<true, 4>)
                        : (u16 ? k_kind_insert<false, 2> : walk ? k_kind_insert<false, 0> : k_kind_insert<false, 4>);
        if (T)
            hipLaunchKernelGGL(kins, dim3(cdiv(T, KB)), dim3(KB), 0, st, koff, kops, (const uint16_t*)g->rs16.p, g->w_t.p,
                               T, g->ht_key.p, g->ht_cr.p, g->slot_of.p, (uint64_t)(cap - 1), seed,
                               chk ? g->ht_chk.p : (uint64_t*)nullptr, hmask);
        MR_DEBUG_CHECK(ctx, "k_kind_insert");
        if (T && u16)
            hipLaunchKernelGGL(k_kind_verify<uint16_t>, dim3(cdiv(T, 256)), dim3(256), 0, st, koff,
                               (const uint16_t*)g->rs16.p, g->w_t.p, T, g->ht_cr.p, g->slot_of.p, g->kind.p, g->flag.p,
                               g->krep.p);
        else if (T)
            hipLaunchKernelGGL(k_kind_verify<int32_t>, dim3(cdiv(T, 256)), dim3(256), 0, st, koff, kops, g->w_t.p, T,
                               g->ht_cr.p, g->slot_of.p, g->kind.p, g->flag.p, g->krep.p);
        MR_DEBUG_CHECK(ctx, "k_kind_verify");
    } else if (T) {
        // partitions P = 2^pb >= T / KP_MEAN by the hash's top bits (records <= T)
        const int pb = bits_for((uint64_t)(cdiv(T, KP_MEAN) - 1));
        const int64_t P = (int64_t)1 << pb;
        const int32_t nb = cdiv(T, KB);
        const size_t R = (size_t)nb * KB;
        DBuf<KRec> rec, e;
        DBuf<int32_t> nrec, rec_of, rpos, hist;
        DBuf<uint32_t> eslot;
        DBuf<int64_t> pstart, tmp;
        DBuf<unsigned long long> cur;
        MR_TRY(rec.alloc(ctx, R));
        MR_TRY(e.alloc(ctx, (size_t)T));
        MR_TRY(nrec.alloc(ctx, (size_t)nb));
        MR_TRY(rec_of.alloc(ctx, (size_t)T));
        MR_TRY(pstart.alloc(ctx, (size_t)P + 1));
        // The two-pass grouping (k_kp1_*, k_kp2; no device atomic per record) at every size: its
        // records carry their block-order slot (eslot), k_kind_part writes each class back there and
        // k_kind_final reads it in block order -- one random 8-B write per record, where the
        // per-record cursor scatter (k_kind_rscatter: a returning atomic and a random 16-B write per
        // record, then a random read per trace; 7.4 ms of C5's 100M records) took three.
        // MR_KIND_GROUP=cursor (A/B, read per call) forces the cursor form.
        const char* kge = getenv("MR_KIND_GROUP");
        const bool cursor = kge && !strcmp(kge, "cursor");
        auto krec = u16 ? k_kind_rec<2> : walk ? k_kind_rec<0> : k_kind_rec<4>;
        if (cursor) {
            MR_TRY(rpos.alloc(ctx, R));
            MR_TRY(hist.zero(ctx, (size_t)P));
            MR_TRY(cur.alloc(ctx, (size_t)P));
            MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(P)));
            hipLaunchKernelGGL(krec, dim3(nb), dim3(KB), 0, st, koff, kops, (const uint16_t*)g->rs16.p, g->w_t.p, T,
                               seed, hmask, pb, rec.p, nrec.p, rec_of.p, hist.p);
            MR_TRY(mr_exclusive_scan_i32(ctx, hist.p, pstart.p, P, tmp.p));
            MR_TRY_HIP(ctx, hipMemcpyAsync(cur.p, pstart.p, (size_t)P * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(k_kind_rscatter, dim3(cdiv((int64_t)R, 256)), dim3(256), 0, st, rec.p, nrec.p,
                               (int32_t)std::min<size_t>(R, 0x7fffffff), pb, cur.p, e.p, rpos.p);
        } else {
            const int b1 = std::min(pb, KP1_B), nbk = 1 << b1, nf = 1 << (pb - b1);
            const int32_t ntile = (int32_t)cdiv((int64_t)R, KT);
            const int64_t nc = (int64_t)nbk * ntile;
            DBuf<int32_t> tcnt;
            DBuf<int64_t> toff;
            DBuf<KRec> r1;
            DBuf<uint32_t> s1;
            MR_TRY(tcnt.alloc(ctx, (size_t)nc));
            MR_TRY(toff.alloc(ctx, (size_t)nc + 1));
            MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(nc)));
            MR_TRY(r1.alloc(ctx, (size_t)T));
            MR_TRY(s1.alloc(ctx, (size_t)T));
            hipLaunchKernelGGL(krec, dim3(nb), dim3(KB), 0, st, koff, kops, (const uint16_t*)g->rs16.p, g->w_t.p, T,
                               seed, hmask, pb, rec.p, nrec.p, rec_of.p, (int32_t*)nullptr);
            hipLaunchKernelGGL(k_kp1_count, dim3(ntile), dim3(KT_T), 0, st, rec.p, nrec.p, (int64_t)R, b1, ntile, tcnt.p);
            MR_TRY(mr_exclusive_scan_i32(ctx, tcnt.p, toff.p, nc, tmp.p));
            hipLaunchKernelGGL(k_kp1_scatter, dim3(ntile), dim3(KT_T), 0, st, rec.p, nrec.p, (int64_t)R, b1, ntile,
                               toff.p, r1.p, s1.p);
            const size_t lds2 = (size_t)KP2_T * sizeof(int64_t) + (size_t)nf * sizeof(uint32_t);
            MR_TRY(eslot.alloc(ctx, (size_t)T));
            hipLaunchKernelGGL(k_kp2, dim3(nbk), dim3(KP2_T), lds2, st, r1.p, s1.p, toff.p, pb, b1, ntile, e.p, eslot.p,
                               pstart.p);
            MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (the level-1 buffers leave scope)
        }
        hipLaunchKernelGGL(k_kind_part, dim3((uint32_t)P), dim3(KP_B), 0, st, pstart.p, e.p, g->flag.p,
                           cursor ? nullptr : eslot.p, rec.p);
        // the classes: through rpos into e (cursor form) or in block order in rec (two-pass form)
        const int32_t* rp = cursor ? rpos.p : nullptr;
        const KRec* cls = cursor ? e.p : rec.p;
        if (u16)
            hipLaunchKernelGGL(k_kind_final<uint16_t>, dim3(cdiv(T, 256)), dim3(256), 0, st, rec_of.p, rp, cls, koff,
                               (const uint16_t*)g->rs16.p, g->w_t.p, T, g->kind.p, g->flag.p, g->krep.p);
        else
            hipLaunchKernelGGL(k_kind_final<int32_t>, dim3(cdiv(T, 256)), dim3(256), 0, st, rec_of.p, rp, cls, koff,
                               kops, g->w_t.p, T, g->kind.p, g->flag.p, g->krep.p);
        MR_DEBUG_CHECK(ctx, "k_kind_part");
    }
    return MR_OK;
}

// Kinds with representatives: g->kind and g->krep under the seed sequence of mr_pagerank_batch_impl,
// a 64-bit key collision rerun with the next seed.  call_reset: the reset of a ranking's set-up
// (pr_reset_launch over the T traces: pref and c_t cleared too, as the kind-compressed ranking does
// ahead of its own); else only the words the kinds themselves need (the hash table, flag, scal).
static int kinds_with_reps(mr_ctx* ctx, mr_graph* g, bool call_reset) {
    hipStream_t st = ctx->stream;
    const int32_t T = g->T, N = g->N;
    uint64_t cap = 1;
    while (cap < 2ull * (uint64_t)T) cap <<= 1;
    const bool ktab = (int64_t)T < kind_part_min();
    if (!ktab) cap = 0;
    MR_TRY(g->kind.alloc(ctx, (size_t)T));
    MR_TRY(g->krep.alloc(ctx, (size_t)T));
    if (call_reset) {
        MR_TRY(g->pref.alloc(ctx, (size_t)T));
        MR_TRY(g->c_t.alloc(ctx, (size_t)T));
    }
    MR_TRY(g->flag.alloc(ctx, 8));
    MR_TRY(g->scal.alloc(ctx, 8));
    if (ktab) {
        MR_TRY(g->ht_key.alloc(ctx, cap));
        MR_TRY(g->ht_cr.alloc(ctx, cap));
        MR_TRY(g->slot_of.alloc(ctx, (size_t)T));
    }
    bool ok = false;
    for (int a = 0; a < 4 && !ok; ++a) {
        pr_reset_launch(ctx, call_reset ? T : 0, (int64_t)cap, N, g->pref.p, g->c_t.p, g->ht_key.p, g->ht_cr.p, g->flag.p,
                        g->scal.p);
        MR_TRY(graph_kinds(ctx, g, false, ktab, cap, kind_seed(a), kind_hmask(a)));
        int32_t hf[4];
        MR_TRY(g->flag.download(ctx, hf, 4));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
        if (hf[2] & 1) return mr_fail(ctx, MR_ERR_STATE, "trace kinds: a partition exceeded its table");
        ok = !(hf[0] & 1);
    }
    if (!ok) return mr_fail(ctx, MR_ERR_STATE, "trace-kind hash collision under 4 seeds");
    g->krep_ok = true;
    return MR_OK;
}

// mr_internal.h: the representatives for the exemplars' one-per-kind selection, after a ranking.  The
// kinds run on buffers of their own, swapped into the graph for the step: the class sizes a ranking
// left (kind), its flag and sum words and its hash table are what they were when the step returns,
// pref and c_t are never touched -- k_trace_rank, mr_graph_fetch and the next ranking read them.
int mr_kind_reps_ensure(mr_ctx* ctx, mr_graph* g) {
    if (g->krep_ok && g->krep.p) return MR_OK;
    const int64_t* koff = g->rs_is_sr ? g->rs_off.p : g->srt_off.p;
    if (!koff || !g->w_t.p) return mr_fail(ctx, MR_ERR_STATE, "trace kinds: the graph has no trace-major incidence");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    struct Swap {   // the graph's own buffers aside while the kinds run, back on every way out
        mr_graph* g;
        DBuf<double> kind, scal;
        DBuf<int32_t> flag, slot_of;
        DBuf<unsigned long long> ht_key;
        DBuf<KCnt> ht_cr;
        void flip() {
            g->kind.swap(kind);
            g->scal.swap(scal);
            g->flag.swap(flag);
            g->slot_of.swap(slot_of);
            g->ht_key.swap(ht_key);
            g->ht_cr.swap(ht_cr);
        }
        explicit Swap(mr_graph* g_) : g(g_) { flip(); }
        ~Swap() { flip(); }
    } aside(g);
    return kinds_with_reps(ctx, g, false);   // (synchronised: its last read-back waited for the stream)
}

// MR_PR_KIND_COMPRESS (§8(f) f4): kinds of g with each trace's class representative, then a graph
// of the K representatives (multiplicities carried in q and in the preference sums), ranked
// by the same fused iteration; its weights are g's.  Graphs off the fused path (or with
// pr_trace != operation_trace) rank uncompressed.
static int kind_compressed_pagerank(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters,
                                    int precision, uint32_t flags) {
    const uint32_t plain = flags & ~(uint32_t)MR_PR_KIND_COMPRESS;
    if (!ctx || !g || g->ctx != ctx) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank: bad arguments");
    const int32_t T = g->T, N = g->N;
    if (!g->fused || !g->rs_is_sr || !g->pr_identity || T == 0 || N == 0)
        return mr_pagerank_batch_impl(ctx, &g, &anomaly, 1, d, alpha, iters, precision, plain);
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the representatives' graph depends on g's structure only (built, never changed): a later call
    // ranks the kept one (its preference and iteration state are set up per call as usual).
    // MR_KC_NOCACHE: rebuild every call (read per call)
    auto rank_kc = [&](mr_graph* gcp) -> int {
        gcp->phi = g->phi;
        MR_TRY(mr_pagerank_batch_impl(ctx, &gcp, &anomaly, 1, d, alpha, iters, precision, plain));
        MR_TRY(g->weight.alloc(ctx, (size_t)N));
        MR_TRY(g->sn.alloc(ctx, (size_t)N));
        MR_TRY_HIP(ctx, hipMemcpyAsync(g->weight.p, gcp->weight.p, (size_t)N * 8, hipMemcpyDeviceToDevice, st));
        MR_TRY_HIP(ctx, hipMemcpyAsync(g->sn.p, gcp->sn.p, (size_t)N * 8, hipMemcpyDeviceToDevice, st));
        return MR_OK;
    };
    if (g->kc && getenv("MR_KC_NOCACHE") == nullptr) return rank_kc(g->kc.get());
    g->kc.reset();
    MR_TRY(kinds_with_reps(ctx, g, true));
    // ---- the representatives' graph
    DBuf<int32_t> fl, rep, cnt;
    DBuf<int64_t> pos, tmp;
    MR_TRY(fl.alloc(ctx, (size_t)T));
    MR_TRY(pos.alloc(ctx, (size_t)T + 1));
    MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(T)));
    hipLaunchKernelGGL(k_kc_flags, dim3(cdiv(T, 256)), dim3(256), 0, st, g->krep.p, T, fl.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, fl.p, pos.p, T, tmp.p));
    int64_t K = 0;
    MR_TRY_HIP(ctx, hipMemcpyAsync(&K, pos.p + T, sizeof K, hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    std::unique_ptr<mr_graph> gc(new mr_graph());
    gc->ctx = ctx;
    gc->N = N;
    gc->T = (int32_t)K;
    gc->T_all = T;   // v0 = 1 / (N + T) over every trace (pagerank.py:118-119)
    gc->E = g->E;
    MR_TRY(rep.alloc(ctx, (size_t)K));
    MR_TRY(cnt.alloc(ctx, (size_t)K));
    MR_TRY(gc->len_t.alloc(ctx, (size_t)K));
    MR_TRY(gc->mult.alloc(ctx, (size_t)K));
    hipLaunchKernelGGL(k_kc_reps, dim3(cdiv(T, 256)), dim3(256), 0, st, fl.p, pos.p, T, g->rs_off.p, g->len_t.p,
                       g->kind.p, rep.p, gc->len_t.p, gc->mult.p, cnt.p);
    MR_TRY(gc->rs_off.alloc(ctx, (size_t)K + 1));
    MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(K)));
    MR_TRY(mr_exclusive_scan_i32(ctx, cnt.p, gc->rs_off.p, K, tmp.p));
    int64_t nnz = 0;
    MR_TRY_HIP(ctx, hipMemcpyAsync(&nnz, gc->rs_off.p + K, sizeof nnz, hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    MR_TRY(gc->rs_ops.alloc(ctx, (size_t)nnz));
    hipLaunchKernelGGL(k_kc_ops, dim3(cdiv(K, 256)), dim3(256), 0, st, rep.p, gc->rs_off.p, (int32_t)K, g->rs_off.p,
                       g->rs_ops.p, gc->rs_ops.p);
    MR_TRY(gc->len_o.alloc(ctx, (size_t)N));
    MR_TRY(gc->nchild.alloc(ctx, (size_t)N));
    MR_TRY(gc->ss_off.alloc(ctx, (size_t)N + 1));
    MR_TRY(gc->ss_par.alloc(ctx, (size_t)std::max<int64_t>(g->E, 1)));
    MR_TRY_HIP(ctx, hipMemcpyAsync(gc->len_o.p, g->len_o.p, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    MR_TRY_HIP(ctx, hipMemcpyAsync(gc->nchild.p, g->nchild.p, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    MR_TRY_HIP(ctx, hipMemcpyAsync(gc->ss_off.p, g->ss_off.p, ((size_t)N + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (g->E) MR_TRY_HIP(ctx, hipMemcpyAsync(gc->ss_par.p, g->ss_par.p, (size_t)g->E * 4, hipMemcpyDeviceToDevice, st));
    gc->rs_is_sr = true;
    gc->pr_identity = true;
    gc->n_pr = (int32_t)K;
    gc->nnz_sr = gc->nnz_rs = nnz;
    gc->kinds_given = true;   // (before the prepare: its layout is then the stable sort)
    MR_TRY(mr_graph_prepare(ctx, gc.get()));
    if (!gc->fused)
        return mr_pagerank_batch_impl(ctx, &g, &anomaly, 1, d, alpha, iters, precision, plain);
    MR_TRY(gc->mw_tp.alloc(ctx, (size_t)K));
    hipLaunchKernelGGL(k_kc_mw, dim3(cdiv(K, 256)), dim3(256), 0, st, gc->tperm.p, gc->w_tp.p, gc->mult.p, (int32_t)K,
                       gc->mw_tp.p);
    DBuf<int64_t> tm;
    MR_TRY(tm.alloc(ctx, (size_t)std::max(gc->n_wt, 1)));
    hipLaunchKernelGGL(k_kc_tile_mult, dim3(cdiv(gc->n_wt, 256)), dim3(256), 0, st, gc->tperm.p, gc->mult.p, (int32_t)K,
                       gc->n_wt, tm.p);
    gc->tile_mult_h.assign((size_t)gc->n_wt, 0);
    MR_TRY(tm.download(ctx, gc->tile_mult_h.data(), (size_t)gc->n_wt));
    MR_TRY(gc->kind.alloc(ctx, (size_t)K));   // the class sizes, as the preference reads them
    MR_TRY_HIP(ctx, hipMemcpyAsync(gc->kind.p, gc->mult.p, (size_t)K * 8, hipMemcpyDeviceToDevice, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    MR_TRY(rank_kc(gc.get()));
    g->kc_kinds = K;
    g->kc = std::move(gc);
    return MR_OK;
}

// a ranking asked with MR_PR_KIND_COMPRESS: the trace vector lives on the representatives' graph (or,
// for a graph that ranked uncompressed, on g -- the record says "compressed" either way: what a caller
// may read afterwards follows from the flag it passed, not from the graph's form)
int kind_compressed_call(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters, int precision,
                                uint32_t flags) {
    if (g) g->rk_ok = g->trank_ok = false;
    MR_TRY(kind_compressed_pagerank(ctx, g, anomaly, d, alpha, iters, precision, flags));
    g->rk_ok = g->rk_kc = true;
    g->rk_fp32 = precision == MR_FP32;
    g->rk_iters = iters;
    g->rk_d = d;
    g->trank_ok = false;
    return MR_OK;
}
