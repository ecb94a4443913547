// The set-up of a K2 call, everything before the iterations: the preference vector
// (pagerank.py:68-85, T4), the iteration state (v0 = 1 / (N + traces), pagerank.py:118-119) and the
// per-call words, per graph (pagerank_setup), for many window graphs in one launch per step
// (pagerank_setup_batch), and for window graphs in layout order (mr_lo_prepare_batch); set-ups made
// ahead of the call (mr_pagerank_presetup).  The kinds themselves: mr_pr_kinds.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "mr_iter_dev.h"
#include "mr_pr_dev.h"
#include "mr_pr_internal.h"

namespace {

// every per-call word of the kinds and the preference cleared (thread i: word i of each buffer)
__device__ __forceinline__ void pr_reset_body(int64_t i, int32_t T, int64_t cap, float* pref, float* c_t,
                                              unsigned long long* hk, KCnt* cr, int32_t* flag, double* scal) {
    if (i < T) {
        pref[i] = 0.0f;
        c_t[i] = 0.0f;
    }
    if (i < cap) {
        hk[i] = 0ull;
        cr[i] = KCnt{0u, 0x7fffffff};
    }
    if (i < 8) flag[i] = 0;
    if (i < 8) scal[i] = 0.0;
}
__global__ void k_pr_reset(int32_t T, int64_t cap, int32_t N, float* pref, float* c_t, unsigned long long* hk, KCnt* cr, int32_t* flag,
                           double* scal) {
    pr_reset_body((int64_t)blockIdx.x * blockDim.x + threadIdx.x, T, cap, pref, c_t, hk, cr, flag, scal);
}

// ---------------------------------------------------------------- preference (pagerank.py:68-85)
// sums over pr_trace entries: [0] sum 1/k, [1] sum 1/len; block partials then one fixed-order pass
// mult (kind-compressed graphs): trace i stands for mult[i] traces of its kind
// the block's two sums, in block_sum order, into part[2 blk], part[2 blk + 1]
__device__ __forceinline__ void pref_partial_store(int32_t blk, double a, double b, double* part) {
    __shared__ double red[TB / WAVE];
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        part[2 * blk] = a;
        part[2 * blk + 1] = b;
    }
}
__device__ __forceinline__ void pref_partial_body(int32_t blk, const double* kind, const int32_t* pr_trace,
                                                  const int32_t* pr_len, const int32_t* len_t, int32_t n_pr,
                                                  const double* mult, double* part, int32_t* flag) {
    double a = 0.0, b = 0.0;
    int32_t i = blk * blockDim.x + threadIdx.x;
    if (i < n_pr) {
        int32_t t = pr_trace ? pr_trace[i] : i;
        int32_t ln = pr_len ? pr_len[i] : len_t[t];
        a = 1.0 / kind[t];
        if (ln == 0) atomicOr(flag + 1, 1);   // 1.0/len(pr_trace[t]) -> ZeroDivisionError (word 1)
        b = ln ? 1.0 / (double)ln : 0.0;
        if (mult) {
            a *= mult[t];
            b *= mult[t];
        }
    }
    pref_partial_store(blk, a, b, part);
}
__global__ void k_pref_partial(const double* kind, const int32_t* pr_trace, const int32_t* pr_len,
                               const int32_t* len_t, int32_t n_pr, const double* mult, double* part, int32_t* flag) {
    pref_partial_body((int32_t)blockIdx.x, kind, pr_trace, pr_len, len_t, n_pr, mult, part, flag);
}

// (a last-block total inside k_pref_partial was measured slower: the per-block release fence
// writes back the XCD's L2, 21 us against 6.7 + 5.6 us for the two launches)
// one block of 1024 threads: the nb block partials, strided, then block_sum
__device__ __forceinline__ void pref_total_body(const double* part, int32_t nb, double* scal) {
    __shared__ double red[1024 / WAVE];
    double a = 0.0, b = 0.0;
    for (int32_t i = threadIdx.x; i < nb; i += blockDim.x) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        scal[2] = a;
        scal[3] = b;
    }
}
__global__ void k_pref_total(const double* part, int32_t nb, double* scal) { pref_total_body(part, nb, scal); }

// reference order, one thread (MR_PR_EXACT_SUMS, T7)
__global__ void k_pref_total_exact(const double* kind, const int32_t* pr_trace, const int32_t* pr_len,
                                   const int32_t* len_t, int32_t n_pr, double* scal) {
    if (threadIdx.x || blockIdx.x) return;
    double a = 0.0, b = 0.0;
    for (int32_t i = 0; i < n_pr; ++i) {
        int32_t t = pr_trace ? pr_trace[i] : i;
        int32_t ln = pr_len ? pr_len[i] : len_t[t];
        a += 1.0 / kind[t];
        b += ln ? 1.0 / (double)ln : 0.0;
    }
    scal[2] = a;
    scal[3] = b;
}

// the preference of a trace of kind size k and ln spans (scal[2] = sum 1/k, scal[3] = sum 1/len)
__device__ __forceinline__ double pref_value(double k, int32_t ln, const double* scal, int anomaly, double phi) {
    return !anomaly ? 1.0 / k / scal[2]                                               // :74
                    : 1.0 / (k / scal[2] * phi + 1.0 / (double)ln) / scal[3] * phi;   // :80-85 (phi = 0.5)
}

// tperm (k_tr_a graphs with pr_trace = operation_trace): thread i is position i, and c_t goes to
// c_tp[i] too (formerly k_tr_gather)
__global__ void k_pref_apply(const double* kind, const int32_t* pr_trace, const int32_t* pr_len,
                             const int32_t* len_t, int32_t n_pr, const double* scal, int anomaly,
                             float cd, double phi, float* pref, float* c_t, const int32_t* tperm, float* c_tp) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pr) return;
    int32_t t = tperm ? tperm[i] : pr_trace ? pr_trace[i] : i;
    int32_t ln = pr_len ? pr_len[i] : len_t[t];
    float vf = (float)pref_value(kind[t], ln, scal, anomaly, phi);
    pref[t] = vf;
    c_t[t] = cd * vf;   // (1.0 - d) * v: float32 array times a Python float stays float32 (T4)
    if (tperm) c_tp[i] = cd * vf;
}

// Large k_tr_a graphs (pr_trace = operation_trace): the same values in TRACE order -- kind[t],
// len_t[t] read and pref[t] written coalesced, only c_tp scattered (through tpos, the inverse of
// tperm).  The position-order form above gathers kind / len_t and scatters pref / c_t at random
// t: four random streams per trace, 11 ms at C5's 100M traces.  c_t itself
// is not written: the fused iteration reads only c_tp (the batched set-up passes c_t and has it).
__device__ __forceinline__ void pref_apply_t_body(int32_t t, const double* __restrict__ kind,
                                                  const int32_t* __restrict__ len_t, int32_t T,
                                                  const double* __restrict__ scal, int anomaly, float cd, double phi,
                                                  float* __restrict__ pref, const int32_t* __restrict__ tpos,
                                                  float* __restrict__ c_tp, float* __restrict__ c_t) {
    if (t >= T) return;
    const float vf = (float)pref_value(kind[t], len_t[t], scal, anomaly, phi);
    pref[t] = vf;
    if (c_t) c_t[t] = cd * vf;
    c_tp[tpos[t]] = cd * vf;   // (1.0 - d) * v in float32 (T4)
}
__global__ void k_pref_apply_t(const double* __restrict__ kind, const int32_t* __restrict__ len_t, int32_t T,
                               const double* __restrict__ scal, int anomaly, float cd, double phi, float* __restrict__ pref,
                               const int32_t* __restrict__ tpos, float* __restrict__ c_tp) {
    pref_apply_t_body((int32_t)(blockIdx.x * blockDim.x + threadIdx.x), kind, len_t, T, scal, anomaly, cd, phi, pref, tpos,
                      c_tp, nullptr);
}
__global__ void k_inv_perm(const int32_t* __restrict__ perm, int32_t n, int32_t* __restrict__ inv) {
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) inv[perm[p]] = p;
}
__global__ void k_tr_gather(const float* src, const int32_t* tperm, int32_t T, float* dst) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < T) dst[p] = src[tperm[p]];
}

// ---------------------------------------------------------------- iteration state
// (the maxima ring -- MSH, MSLOT_WORDS, bits2d / d2bits: mr_iter_dev.h)
__device__ __forceinline__ int32_t cdiv_d(int32_t a, int32_t b) { return (a + b - 1) / b; }
// The iteration state (thread i: word i of each buffer); v0 = 1 / (N + traces of the whole graph,
// all shards), pagerank.py:118-119.
// perm (relabelled fused graphs): su is kept in the kernel's op labels, su[new] = u_o[perm[new]] s
// w_t: in position order for k_tr_a (w_tp: q is then indexed by position), else by trace
// su32 (fp32 wide graphs): su also as floats in suf0 / suf1
__device__ __forceinline__ void iter_init_body(int64_t i, int32_t N, int32_t T, double v0, const float* w_t,
                                               const double* mw, const float* u_o, const int32_t* perm, double* sp0,
                                               double* su0, double* su1, double* q64, float* q32, int fp32,
                                               unsigned long long* mslot, int su32, float* suf0, float* suf1) {
    if (i < N) {
        sp0[i] = v0;
        const double su = (double)u_o[perm ? perm[i] : i] * v0;
        su0[i] = su32 ? (double)(float)su : su;   // (fp32 wide graphs: k_tr_a's float copies are exact)
        if (su32) suf0[i] = (float)su;
    }
    if (i >= N && i < N + TR_PAD) su0[i] = su1[i] = 0.0;   // the fused walks' pad slots
    if (su32 && i >= N && i < N + TR_PAD) suf0[i] = suf1[i] = 0.0f;
    if (i < T) {
        const double q = (mw ? mw[i] : (double)w_t[i]) * v0;   // mw: w_t times the kind's multiplicity
        if (fp32) q32[i] = (float)q; else q64[i] = q;
    }
    // M_s(0) = M_r(0) = 1: s_0, r_0 are used as they are; slots 1, 2 start cleared
    if (i < MSLOT_WORDS) mslot[i] = i < 2 * MSH ? d2bits(1.0) : 0ull;
}
// pr_reset_body and iter_init_body in one launch (the iteration state depends on nothing the kinds
// or the preference compute); T_all: traces of the whole graph (all shards)
__global__ void k_pr_reset_init(int32_t T, int64_t cap, int32_t N, float* pref, float* c_t, unsigned long long* hk,
                                KCnt* cr, int32_t* flag, double* scal, const float* w_t, const double* mw,
                                const float* u_o, int64_t T_all, double* sp0, double* su0, double* su1, double* q64,
                                float* q32, int fp32, unsigned long long* mslot, const int32_t* perm, int su32,
                                float* suf0, float* suf1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    pr_reset_body(i, T, cap, pref, c_t, hk, cr, flag, scal);
    iter_init_body(i, N, T, 1.0 / (double)((int64_t)N + T_all), w_t, mw, u_o, perm, sp0, su0, su1, q64, q32, fp32, mslot,
                   su32, suf0, suf1);
}
// ---------------------------------------------------------------- batched set-up
// The set-up of many window graphs (reset + iteration state, kinds, preference) as ONE launch per
// step for all of them (a block range per graph, as the iteration's launches are), instead of six
// launches per graph from the windows' host threads.  Same bodies, same results.
struct SDev {
    int32_t T, N, anomaly, fp32;
    int64_t cap, T_all;
    float cd;
    double phi;                                 // the anomaly preference's 0.5 (pagerank.py:82-84)
    int32_t b_reset, b_kins, b_kver, b_pref;   // the graph's first block in each launch
    float *pref, *c_t, *c_tp;
    const int32_t *tperm, *tpos;
    unsigned long long* hk;
    KCnt* cr;
    int32_t *slot_of, *flag;
    double *kind, *scal, *ppart;
    const float *w_t, *w_tq, *u_o;              // w_t by trace; in q's order (position order for k_tr_a graphs)
    double *sp0, *su0, *su1, *q64;
    float* q32;
    unsigned long long* mslot;
    const int32_t* perm;
    const int64_t* off;
    const uint16_t* o16;
    const int32_t* len_t;
};
__global__ void k_reset_init_b(const SDev* __restrict__ sd, int32_t ng) {
    const SDev& G = sd[block_owner<SDev, &SDev::b_reset>(sd, ng, (int32_t)blockIdx.x)];
    const int64_t i = (int64_t)((int32_t)blockIdx.x - G.b_reset) * blockDim.x + threadIdx.x;
    pr_reset_body(i, G.T, G.cap, G.pref, G.c_t, G.hk, G.cr, G.flag, G.scal);
    // (no wide graphs here, setup_batchable: no float copies of su)
    iter_init_body(i, G.N, G.T, 1.0 / (double)((int64_t)G.N + G.T_all), G.w_tq, nullptr, G.u_o, G.perm, G.sp0, G.su0,
                   G.su1, G.q64, G.q32, G.fp32, G.mslot, 0, nullptr, nullptr);
}
__global__ void __launch_bounds__(KB) k_kind_insert_b(const SDev* __restrict__ sd, int32_t ng, uint64_t seed,
                                                      uint64_t hmask) {
    const SDev& G = sd[block_owner<SDev, &SDev::b_kins>(sd, ng, (int32_t)blockIdx.x)];
    kind_insert_body<false, 2>((int32_t)blockIdx.x - G.b_kins, G.off, nullptr, G.o16, G.w_t, G.T, G.hk, G.cr,
                                  G.slot_of, (uint64_t)(G.cap - 1), seed, nullptr, hmask);
}
__global__ void k_kind_verify_b(const SDev* __restrict__ sd, int32_t ng) {
    const SDev& G = sd[block_owner<SDev, &SDev::b_kver>(sd, ng, (int32_t)blockIdx.x)];
    kind_verify_body<uint16_t>(((int32_t)blockIdx.x - G.b_kver) * blockDim.x + threadIdx.x, G.off, G.o16, G.w_t, G.T, G.cr,
                               G.slot_of, G.kind, G.flag, nullptr);
}
__global__ void k_pref_partial_b(const SDev* __restrict__ sd, int32_t ng) {
    const SDev& G = sd[block_owner<SDev, &SDev::b_pref>(sd, ng, (int32_t)blockIdx.x)];
    pref_partial_body((int32_t)blockIdx.x - G.b_pref, G.kind, nullptr, nullptr, G.len_t, G.T, nullptr, G.ppart, G.flag);
}
__global__ void k_pref_total_b(const SDev* __restrict__ sd) {   // block g: graph g
    const SDev& G = sd[blockIdx.x];
    pref_total_body(G.ppart, cdiv_d(G.T, TB), G.scal);
}
// in trace order (as k_pref_apply_t): the per-trace reads and writes are coalesced, the one
// scattered store is c_tp at the trace's position (tpos, the inverse of tperm)
__global__ void k_pref_apply_b(const SDev* __restrict__ sd, int32_t ng) {
    const SDev& G = sd[block_owner<SDev, &SDev::b_pref>(sd, ng, (int32_t)blockIdx.x)];
    pref_apply_t_body(((int32_t)blockIdx.x - G.b_pref) * blockDim.x + threadIdx.x, G.kind, G.len_t, G.T, G.scal, G.anomaly,
                      G.cd, G.phi, G.pref, G.tpos, G.c_tp, G.c_t);
}

// ---------------------------------------------------------------- window graphs in layout order
// (mr_lo_prepare_batch) A graph whose positions come from its table's layout order (pinv[p] =
// the layout index of position p): chunk offsets, the lane-interleaved ids (the table's u16 codes
// relabelled to node ids: node_of_code), w_t / span count / kind class size by position and the
// preference partials, then the totals, then the preference and iteration state -- the work of
// k_graph_consts .. k_tr_fill and k_reset_init .. k_pref_apply for these graphs, in four launches.
constexpr int LO_NOC_MAX = 4096;   // (mr_lo_fits: tables of <= NS_PMAX pod-ops)
struct LDev {
    int32_t T, N, W, anomaly, fp32, NP;
    int32_t b_cs, n_cs, b_fill, nbp, b_app;   // first block in each launch; partial blocks
    int64_t st_off;
    float cd;
    double phi, v0;
    const int32_t* pinv;
    const int64_t* lo_off;
    const uint16_t* lo16;
    const int32_t *lo_len, *lo_kid, *noc;
    const uint32_t* kcnt;
    int64_t* c64;
    int32_t* coff;
    uint16_t* tids;
    float *w_tp, *c_tp;
    double* kind;
    int32_t* lenp;
    uint8_t* trun;
    double *ppart, *scal;
    int32_t* flag;
    unsigned long long* mslot;
    double *sp0, *su0, *su1, *q64;
    float* q32;
    const float* u_o;
};
__global__ void __launch_bounds__(TS_T) k_lo_cs_b(const LDev* __restrict__ ld, int32_t n, unsigned long long* st,
                                                 uint64_t epoch) {
    const LDev& G = ld[block_owner<LDev, &LDev::b_cs>(ld, n, (int32_t)blockIdx.x)];
    tr_chunk_scan_body((int32_t)blockIdx.x - G.b_cs, G.n_cs, G.pinv, G.lo_off, G.T, G.W, G.c64, G.coff, st + G.st_off,
                       epoch);
}
// thread per (tile, lane) = position: as tr_fill_body (the trace rotated by its index mod len, pads
// N + lane), ids relabelled; w_t = fp32(1/len_t), the span count and the class size by position;
// the block's 1/k and 1/len_t sums (pagerank.py:71-78) into ppart
__global__ void __launch_bounds__(256) k_lo_fill_b(const LDev* __restrict__ ld, int32_t n) {
    __shared__ uint16_t lnoc[LO_NOC_MAX];   // the code -> node id table (one LDS read per id)
    const LDev& G = ld[block_owner<LDev, &LDev::b_fill>(ld, n, (int32_t)blockIdx.x)];
    const int32_t blk = (int32_t)blockIdx.x - G.b_fill;
    const int64_t i = (int64_t)blk * 256 + threadIdx.x;
    const int32_t T = G.T, N = G.N;
    for (int32_t c = threadIdx.x; c < G.NP; c += 256) lnoc[c] = (uint16_t)G.noc[c];
    __syncthreads();
    double a = 0.0, b = 0.0;
    if (i < (int64_t)G.W * WAVE) {   // (uniform per wave: a wave is one tile)
        const int32_t k = (int32_t)(i / WAVE), lane = (int32_t)(i % WAVE);
        int64_t e0 = 0, len = 0, rot = 0;
        // every trace rotated by its own layout index mod length.  Run-merged graphs (MR_TR_MERGE=1,
        // trun set; kind compression inside the walk, SURVEY 8(f)4 -- never the headline): runs of
        // identical traces (adjacent positions of one kind class: the layout keeps a class
        // contiguous) share their head's rotation instead, so its members walk the same ids in the
        // same order and k_tr_a lets the head walk for the run
        const int32_t ix = i < T ? G.pinv[i] : -1;
        const int32_t kid = i < T ? G.lo_kid[ix] : -1;
        const int32_t kp = __shfl_up(kid, 1, WAVE);
        const bool hd = lane == 0 || kid < 0 || kid != kp;
        const unsigned long long hm = __ballot(hd);
        const unsigned long long below = hm & (lane == WAVE - 1 ? ~0ull : (2ull << lane) - 1ull);
        const int32_t ixh = __shfl(ix, 63 - __builtin_clzll(below), WAVE);
        // only a tile of the 512-thread walk's short tiers merges (the general loop walks every
        // lane): there its runs share the head's rotation and are marked; a longer tile keeps one
        // rotation per trace (a shared rotation there would put a run's adds on one word at a time)
        const bool mt = G.trun && G.c64[k + 1] - G.c64[k] <= MR_TR_TIERS512;
        if (i < T && G.trun) {
            const unsigned long long above = lane == WAVE - 1 ? 0ull : hm & (~0ull << (lane + 1));
            G.trun[i] = !mt ? (uint8_t)1 : hd ? (uint8_t)((above ? __builtin_ctzll(above) : WAVE) - lane) : (uint8_t)0;
        }
        if (i < T) {
            e0 = G.lo_off[ix];
            len = G.lo_off[ix + 1] - e0;
            rot = len ? (int64_t)((uint32_t)(mt ? ixh : ix) % (uint32_t)len) : 0;
            const int32_t L = G.lo_len[ix];
            const uint32_t kc = G.kcnt[G.lo_kid[ix]];
            G.w_tp[i] = L > 0 ? (float)(1.0 / (double)L) : 0.0f;
            G.lenp[i] = L;
            G.kind[i] = (double)kc;
            a = 1.0 / (double)kc;
            b = L ? 1.0 / (double)L : 0.0;
        }
        const int64_t nc = G.c64[k + 1] - G.c64[k];
        unsigned long long* dst = (unsigned long long*)G.tids + (size_t)G.c64[k] * WAVE + lane;
        constexpr int TF_CH = 4;
        for (int64_t c0 = 0; c0 < nc; c0 += TF_CH) {
            uint16_t idv[4 * TF_CH];
#pragma unroll
            for (int q = 0; q < 4 * TF_CH; ++q) {
                const int64_t e = 4 * c0 + q, jx = rot + e;
                idv[q] = e < len ? lnoc[G.lo16[e0 + (jx >= len ? jx - len : jx)]] : (uint16_t)(N + lane);
            }
#pragma unroll
            for (int u = 0; u < TF_CH; ++u)
                if (c0 + u < nc)
                    dst[(size_t)(c0 + u) * WAVE] = (unsigned long long)idv[4 * u] | (unsigned long long)idv[4 * u + 1] << 16 |
                                                   (unsigned long long)idv[4 * u + 2] << 32 |
                                                   (unsigned long long)idv[4 * u + 3] << 48;
        }
    }
    pref_partial_store(blk, a, b, G.ppart);
}
// (a call that asked for exemplars only) the trace code of every position, tcode[p] = lo_tr[pinv[p]]:
// pinv leaves with the build.  One descriptor per graph, the blocks found as k_lo_apply_b's.
// tkid (a call that asked for one exemplar per kind, else null): tkid[p] = lo_kid[pinv[p]], the
// table's exact kind class of the trace.
struct LTDev {
    const int32_t *pinv, *lo_tr;
    int32_t* tcode;
    int32_t T, b0;
    const int32_t* lo_kid;
    int32_t* tkid;
};
__global__ void __launch_bounds__(256) k_lo_tcode_b(const LTDev* __restrict__ lt, int32_t n) {
    const LTDev& G = lt[block_owner<LTDev, &LTDev::b0>(lt, n, (int32_t)blockIdx.x)];
    const int64_t p = (int64_t)((int32_t)blockIdx.x - G.b0) * 256 + threadIdx.x;
    if (p >= G.T) return;
    const int32_t ix = G.pinv[p];
    G.tcode[p] = G.lo_tr[ix];
    if (G.tkid) G.tkid[p] = G.lo_kid[ix];
}
__global__ void __launch_bounds__(1024) k_lo_total_b(const LDev* __restrict__ ld) {   // block g: graph g
    const LDev& G = ld[blockIdx.x];
    pref_total_body(G.ppart, G.nbp, G.scal);
}
// the preference (pagerank.py:68-85, T4) and the iteration state (k_reset_init_b's) by position;
// of the per-call words only flag[0..3] and scal but [2], [3] (k_lo_total_b's sums) are cleared
__global__ void k_lo_apply_b(const LDev* __restrict__ ld, int32_t n) {
    const LDev& G = ld[block_owner<LDev, &LDev::b_app>(ld, n, (int32_t)blockIdx.x)];
    const int64_t i = (int64_t)((int32_t)blockIdx.x - G.b_app) * blockDim.x + threadIdx.x;
    if (i < G.T) {
        const float vf = (float)pref_value(G.kind[i], G.lenp[i], G.scal, G.anomaly, G.phi);
        G.c_tp[i] = G.cd * vf;   // (1.0 - d) * v in float32 (T4)
    }
    iter_init_body(i, G.N, G.T, G.v0, G.w_tp, nullptr, G.u_o, nullptr, G.sp0, G.su0, G.su1, G.q64, G.q32, G.fp32, G.mslot,
                   0, nullptr, nullptr);
    if (i < 4) G.flag[i] = 0;
    if (i < 8 && i != 2 && i != 3) G.scal[i] = 0.0;
}

}  // namespace

// ------------------------------------------------------------------------------ host side
// k_inv_perm / k_pr_reset for the units that do not own them (wide_prepare; the kind-compressed graph)
void inv_perm_launch(mr_ctx* ctx, const int32_t* perm, int32_t n, int32_t* inv) {
    hipLaunchKernelGGL(k_inv_perm, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, perm, n, inv);
}
void pr_reset_launch(mr_ctx* ctx, int32_t T, int64_t cap, int32_t N, float* pref, float* c_t, unsigned long long* hk,
                     KCnt* cr, int32_t* flag, double* scal) {
    hipLaunchKernelGGL(k_pr_reset, dim3(cdiv(std::max<int64_t>({(int64_t)T, (int64_t)cap, 16}), 256)), dim3(256), 0,
                       ctx->stream, T, cap, N, pref, c_t, hk, cr, flag, scal);
}

// blocks of 256 threads that cover every per-call word of a graph (pr_reset_body, iter_init_body)
static int32_t reset_grid(int32_t T, uint64_t cap, int32_t N) {
    return (int32_t)cdiv(std::max<int64_t>({(int64_t)T, (int64_t)cap, (int64_t)N + TR_PAD, MSLOT_WORDS, 16}), 256);
}
// The buffers of a graph's iteration state and per-call words (all a layout-order graph needs: its
// kinds and preference partials come from its prepare)
static int state_alloc(mr_ctx* ctx, mr_graph* g, bool fp32) {
    const size_t N = (size_t)g->N, T = (size_t)g->T;
    MR_TRY(g->flag.alloc(ctx, 8));
    MR_TRY(g->scal.alloc(ctx, 8));
    MR_TRY(g->mslot.alloc(ctx, MSLOT_WORDS));
    MR_TRY(g->sn.alloc(ctx, N));
    MR_TRY(g->spb[0].alloc(ctx, N));
    MR_TRY(g->spb[1].alloc(ctx, N));
    for (int i = 0; i < 2; ++i) {
        MR_TRY(g->sub[i].alloc(ctx, (size_t)N + TR_PAD));   // [N, N + TR_PAD) = 0: the fused walks' pad slots
        if (fp32 && g->wide) MR_TRY(g->suf[i].alloc(ctx, (size_t)N + TR_PAD));
        if (fp32) MR_TRY(g->q32[i].alloc(ctx, T + 1));   // [T]: k_tr_a's pad slot
        else MR_TRY(g->q64[i].alloc(ctx, T + 1));
    }
    MR_TRY(g->weight.alloc(ctx, N));
    if (g->fused) {
        MR_TRY(g->c_tp.alloc(ctx, std::max<size_t>(T, 1)));
        MR_TRY(g->fx_ssv.alloc(ctx, N));
    } else {
        MR_TRY(g->part.alloc(ctx, (size_t)std::max<int64_t>(g->n_pairs, 1)));
    }
    return MR_OK;
}
// Every buffer of a graph's set-up: the kinds' and the preference's (the hash table of cap slots
// when ktab), then the state's
static int setup_alloc(mr_ctx* ctx, mr_graph* g, bool fp32, bool ktab, uint64_t cap) {
    const size_t T = (size_t)g->T;
    MR_TRY(g->kind.alloc(ctx, T));
    MR_TRY(g->pref.alloc(ctx, T));
    MR_TRY(g->c_t.alloc(ctx, T));
    MR_TRY(g->ppart.alloc(ctx, 2 * (size_t)cdiv(g->n_pr > 0 ? g->n_pr : 1, TB)));
    if (ktab) {
        MR_TRY(g->ht_key.alloc(ctx, cap));
        MR_TRY(g->ht_cr.alloc(ctx, cap));
        MR_TRY(g->slot_of.alloc(ctx, T));
    }
    return state_alloc(ctx, g, fp32);
}
// g is set up for a call with these arguments (and the first kind-hash seed): that call skips its own
static void mark_presetup(mr_graph* g, int anomaly, double d, bool fp32, uint32_t flags) {
    g->pre_ok = true;
    g->rk_ok = g->trank_ok = false;   // (the set-up rewrote the iteration state of the last ranking)
    g->pre_anomaly = anomaly;
    g->pre_d = d;
    g->pre_phi = g->phi;
    g->pre_fp32 = fp32;
    g->pre_flags = flags;
    g->pre_seed = kind_seed(0);
    g->pre_hmask = kind_hmask(0);
}

// ---------------------------------------------------------------- window graphs in layout order
// the iteration state's buffers of a layout-order graph and its LDev set-up fields
static int lo_state(mr_ctx* ctx, mr_graph* g, int anomaly, double d, bool fp32, LDev& v) {
    const int32_t N = g->N, T = g->T;
    MR_TRY(state_alloc(ctx, g, fp32));   // (fused, not wide: mr_lo_prepare_batch)
    v.T = T;
    v.N = N;
    v.anomaly = anomaly;
    v.fp32 = fp32 ? 1 : 0;
    v.cd = (float)(1.0 - d);
    v.phi = g->phi;
    v.v0 = 1.0 / (double)((int64_t)N + T);   // pagerank.py:118-119
    v.nbp = g->lo_nbp;
    v.w_tp = g->w_tp.p;
    v.c_tp = g->c_tp.p;
    v.kind = g->kind.p;
    v.lenp = g->lo_lenp.p;
    v.ppart = g->ppart.p;
    v.scal = g->scal.p;
    v.flag = g->flag.p;
    v.mslot = g->mslot.p;
    v.sp0 = g->spb[0].p;
    v.su0 = g->sub[0].p;
    v.su1 = g->sub[1].p;
    v.q64 = g->q64[0].p;
    v.q32 = g->q32[0].p;
    v.u_o = g->u_o.p;
    return MR_OK;
}
// pagerank_setup of a layout-order graph (a call that did not take its presetup: a group rerun):
// its kind class sizes, span counts and preference partials by position are kept on the graph
static int lo_setup_one(mr_ctx* ctx, mr_graph* g, int anomaly, double d, bool fp32) {
    std::vector<unsigned char> keep(sizeof(LDev), 0);
    LDev& v = *reinterpret_cast<LDev*>(keep.data());
    MR_TRY(lo_state(ctx, g, anomaly, d, fp32, v));
    v.b_app = 0;
    DBuf<LDev> dl;
    MR_TRY(dl.upload(ctx, &v, 1));
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_lo_total_b, dim3(1), dim3(1024), 0, st, dl.p);
    hipLaunchKernelGGL(k_lo_apply_b, dim3(reset_grid(g->T, 0, g->N)), dim3(256), 0, st, dl.p, 1);
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (the host descriptor leaves scope)
    return MR_OK;
}

int mr_lo_prepare_batch(mr_ctx* ctx, mr_graph* const* gs, const mr_spans* const* sps, IxBuild* const* bs,
                        const int* anomaly, int n, double d, int precision, std::vector<unsigned char>& keep,
                        bool keep_tcode, bool keep_tkid) {
    if (n <= 0) return MR_OK;
    const bool fp32 = precision == MR_FP32;
    hipStream_t st = ctx->stream;
    // a trace's ids rotated by its layout index mod length (spreads a shared first op over a tile's
    // id chunks, k_lo_fill_b).  MR_TR_MERGE=1 (read per call; the bench's run-merged side leg and
    // tests): runs of identical traces share their head's rotation and k_tr_a walks each run by its
    // head -- kind compression inside the walk, so never the default: the headline
    // walks every trace.  MR_TR_MERGE=2 (tests): the run rotations without the merged walk, so every
    // lane walks its own trace in its run head's order -- bitwise the merged walk
    const char* mge = getenv("MR_TR_MERGE");
    const int merge = mge ? std::min(std::max(atoi(mge), 0), 2) : 0;
    keep.assign((size_t)n * sizeof(LDev) + (keep_tcode ? (size_t)n * sizeof(LTDev) : 0), 0);
    LDev* hv = reinterpret_cast<LDev*>(keep.data());
    std::vector<DBuf<int64_t>> c64((size_t)n);
    int32_t bcs = 0, bfl = 0, bap = 0;
    int64_t st_words = 0;
    for (int i = 0; i < n; ++i) {
        mr_graph* g = gs[i];
        const mr_spans* sp = sps[i];
        const IxBuild& b = *bs[i];
        const int32_t N = g->N, T = g->T, W = cdiv(T, WAVE);
        const int64_t nnz = g->nnz_sr;
        if (N <= 0 || T <= 0 || N > FX_NMAX || !tr_su_fits(N) || nnz >= (1ll << 31))
            return mr_fail(ctx, MR_ERR_STATE, "mr_lo_prepare_batch: graph outside the layout-order limits");
        g->lo = true;
        g->rs_is_sr = true;
        g->pr_identity = true;
        g->n_pr = T;
        g->traces_nonempty = true;
        g->cov_ready = true;
        g->nhr = 0;
        g->hmask.reset();
        g->relabeled = false;
        g->wide = false;
        g->NA = N;
        g->fused = true;
        g->perm.reset();
        g->rsp.reset();
        g->n_wt = W;
        g->wtile_nw = 0;
        g->coff_h.clear();
        g->n_tiles = 0;
        g->n_pairs = 0;
        g->tpos_ok = false;
        g->lo_nbp = cdiv((int64_t)W * WAVE, 256);
        MR_TRY(g->w_tp.alloc(ctx, (size_t)T));
        MR_TRY(g->kind.alloc(ctx, (size_t)T));
        MR_TRY(g->lo_lenp.alloc(ctx, (size_t)T));
        g->lo_merged = merge;
        if (merge) MR_TRY(g->trun.alloc(ctx, (size_t)T));
        MR_TRY(g->ppart.alloc(ctx, 2 * (size_t)g->lo_nbp));
        MR_TRY(g->coff.alloc(ctx, (size_t)W + 1));
        MR_TRY(c64[(size_t)i].alloc(ctx, (size_t)W + 1));
        const int64_t nch = 2 * (int64_t)W + (nnz / WAVE + 2 * (int64_t)N) / 4 + 2;   // as tr_layout
        MR_TRY(g->tids.alloc(ctx, (size_t)std::max<int64_t>(nch, 1) * WAVE * 4));
        LDev& v = hv[i];
        MR_TRY(lo_state(ctx, g, anomaly[i], d, fp32, v));
        v.W = W;
        v.NP = sp->n_podops;
        v.n_cs = (int32_t)std::max<int64_t>(cdiv((int64_t)W, TS_TILE), 1);
        v.st_off = st_words;
        st_words += v.n_cs;
        v.b_cs = bcs;
        bcs += v.n_cs;
        v.b_fill = bfl;
        bfl += g->lo_nbp;
        v.b_app = bap;
        bap += reset_grid(T, 0, N);   // (no hash table)
        v.pinv = b.pinv.p;
        v.lo_off = sp->lo_off.p;
        v.lo16 = sp->lo16.p;
        v.lo_len = sp->lo_len.p;
        v.lo_kid = sp->lo_kid.p;
        v.noc = b.node_of_code.p;
        v.kcnt = b.kcnt;
        v.c64 = c64[(size_t)i].p;
        v.coff = g->coff.p;
        v.tids = g->tids.p;
        v.trun = merge ? g->trun.p : nullptr;
        mark_presetup(g, anomaly[i], d, fp32, 0);
    }
    DBuf<LDev> dl;
    MR_TRY(dl.upload(ctx, hv, (size_t)n));
    unsigned long long* dst = nullptr;
    uint64_t epoch = 0;
    MR_TRY(mr_dl_status(ctx, st_words, &dst, &epoch));
    hipLaunchKernelGGL(k_lo_cs_b, dim3(bcs), dim3(TS_T), 0, st, dl.p, n, dst, epoch);
    hipLaunchKernelGGL(k_lo_fill_b, dim3(bfl), dim3(256), 0, st, dl.p, n);
    hipLaunchKernelGGL(k_lo_total_b, dim3(n), dim3(1024), 0, st, dl.p);
    hipLaunchKernelGGL(k_lo_apply_b, dim3(bap), dim3(256), 0, st, dl.p, n);
    MR_TRY_HIP(ctx, hipGetLastError());
    if (keep_tcode) {   // the graphs ranked as "normal" (the detector's abnormal traces): the ones exemplars read
        const size_t k0 = (size_t)n * sizeof(LDev);   // (their descriptors behind the LDevs, reserved above)
        int nt = 0;
        for (int i = 0; i < n; ++i) nt += anomaly[i] == 0;
        if (nt) {
            std::vector<LTDev> lt;
            int32_t b0 = 0;
            for (int i = 0; i < n; ++i) {
                if (anomaly[i] != 0) continue;
                MR_TRY(gs[i]->tcode.alloc(ctx, (size_t)gs[i]->T));
                if (keep_tkid) MR_TRY(gs[i]->tkid.alloc(ctx, (size_t)gs[i]->T));
                lt.push_back(LTDev{bs[i]->pinv.p, sps[i]->lo_tr.p, gs[i]->tcode.p, gs[i]->T, b0, sps[i]->lo_kid.p,
                                   keep_tkid ? gs[i]->tkid.p : nullptr});
                b0 += cdiv(gs[i]->T, 256);
            }
            memcpy(keep.data() + k0, lt.data(), lt.size() * sizeof(LTDev));
            DBuf<LTDev> dt;
            MR_TRY(dt.upload(ctx, reinterpret_cast<const LTDev*>(keep.data() + k0), lt.size()));
            hipLaunchKernelGGL(k_lo_tcode_b, dim3(b0), dim3(256), 0, st, (const LTDev*)dt.p, nt);
            MR_TRY_HIP(ctx, hipGetLastError());
        }
    }
    return MR_OK;   // (scratch returns to the stream-ordered pool)
}

int pagerank_setup(mr_ctx* ctx, mr_graph* g, int anomaly, double d, bool fp32, uint32_t flags, bool sharded,
                   uint64_t seed, uint64_t hmask) {
    if (g->lo) return lo_setup_one(ctx, g, anomaly, d, fp32);   // (exact kind classes: no seed to vary)
    hipStream_t st = ctx->stream;
    const int32_t N = g->N, T = g->T;
    // Kinds through a global hash table (k_kind_insert) while it stays cache-resident, and for one
    // shard of a multi-rank graph (the cross-rank merge needs its classes and a check hash per
    // class); larger graphs by partition (k_kind_rec .. k_kind_final: no table of random atomics)
    const bool chk = sharded && ctx->nranks > 1;
    uint64_t cap = 1;
    while (cap < 2ull * (uint64_t)T) cap <<= 1;
    const bool ktab = chk || (int64_t)T < kind_part_min();
    if (!ktab) cap = 0;
    const int32_t n_pr = g->n_pr;
    const int nbp = cdiv(n_pr > 0 ? n_pr : 1, TB);
    MR_TRY(setup_alloc(ctx, g, fp32, ktab, cap));
    const bool tr = g->fused;
    // one launch clears every per-call word (instead of a memset per buffer) and sets the iteration
    // state up (it depends on nothing the kinds / preference compute)
    hipLaunchKernelGGL(k_pr_reset_init, dim3(reset_grid(T, cap, N)),
                       dim3(256), 0, st, T, (int64_t)cap, N, g->pref.p, g->c_t.p, g->ht_key.p, g->ht_cr.p,
                       g->flag.p, g->scal.p, tr ? g->w_tp.p : g->w_t.p, tr ? g->mw_tp.p : nullptr, g->u_o.p,
                       g->T_all > 0 ? g->T_all : (int64_t)T, g->spb[0].p, g->sub[0].p, g->sub[1].p, g->q64[0].p,
                       g->q32[0].p, (int)fp32, g->mslot.p, g->relabeled ? (const int32_t*)g->perm.p : nullptr,
                       (int)(fp32 && g->wide), g->suf[0].p, g->suf[1].p);
    MR_DEBUG_CHECK(ctx, "k_pr_reset_init");
    // ---- kinds (a kind-compressed graph carries its class sizes: kinds_given)
    if (!g->kinds_given) MR_TRY(graph_kinds(ctx, g, chk, ktab, cap, seed, hmask));
    if (chk) MR_TRY(shard_kinds(ctx, g, cap));   // class sizes over all ranks (one rank: already global)
    // ---- preference
    const int32_t* prt = g->pr_identity ? nullptr : g->pr_trace.p;
    const int32_t* prl = g->pr_identity ? nullptr : g->pr_len.p;
    // also with n_pr == 0 (an empty shard): the one block writes the zero partials the sums read
    hipLaunchKernelGGL(k_pref_partial, dim3(nbp), dim3(TB), 0, st, g->kind.p, prt, prl, g->len_t.p, n_pr,
                       g->mult.p, g->ppart.p, g->flag.p);
    if ((flags & MR_PR_EXACT_SUMS) && !sharded && !g->mult.p)
        hipLaunchKernelGGL(k_pref_total_exact, dim3(1), dim3(64), 0, st, g->kind.p, prt, prl, g->len_t.p, n_pr,
                           g->scal.p);
    else
        hipLaunchKernelGGL(k_pref_total, dim3(1), dim3(1024), 0, st, g->ppart.p, nbp, g->scal.p);
    MR_DEBUG_CHECK(ctx, "k_pref");
    if (sharded) MR_TRY(mr_coll_allreduce(ctx, g->scal.p + 2, 2, MR_DT_F64, 0));   // sum(1/k), sum(1/len)
    const float cd = (float)(1.0 - d);
    // k_tr_a graphs whose pr_trace is operation_trace: c_t in position order from the same launch
    const bool fuse_gather = tr && !prt && !prl && n_pr == T;
    // large graphs: trace order, c_tp scattered through the inverse permutation (built once per layout)
    const char* pte = getenv("MR_PREF_T_MIN");   // (tests, A/B; read per call) traces from which the trace-order form runs
    const int64_t pref_t_min = pte ? (int64_t)atoll(pte) : (int64_t)1 << 20;
    if (fuse_gather && T > 0 && (int64_t)T >= pref_t_min) {
        if (!g->tpos_ok) {
            MR_TRY(g->tpos.alloc(ctx, (size_t)T));
            hipLaunchKernelGGL(k_inv_perm, dim3(cdiv(T, 256)), dim3(256), 0, st, g->tperm.p, T, g->tpos.p);
            g->tpos_ok = true;
        }
        hipLaunchKernelGGL(k_pref_apply_t, dim3(cdiv(T, 256)), dim3(256), 0, st, g->kind.p, g->len_t.p, T, g->scal.p,
                           anomaly, cd, g->phi, g->pref.p, g->tpos.p, g->c_tp.p);
        MR_DEBUG_CHECK(ctx, "k_pref_apply_t");
        return MR_OK;
    }
    if (n_pr > 0)
        hipLaunchKernelGGL(k_pref_apply, dim3(nbp), dim3(TB), 0, st, g->kind.p, prt, prl, g->len_t.p, n_pr,
                           g->scal.p, anomaly, cd, g->phi, g->pref.p, g->c_t.p, fuse_gather ? (const int32_t*)g->tperm.p : nullptr,
                           fuse_gather ? g->c_tp.p : nullptr);
    MR_DEBUG_CHECK(ctx, "k_pref_apply");
    if (tr && T && !fuse_gather)
        hipLaunchKernelGGL(k_tr_gather, dim3(cdiv(T, 256)), dim3(256), 0, st, g->c_t.p, g->tperm.p, T, g->c_tp.p);
    return MR_OK;
}

// Can pagerank_setup of g run inside a batched set-up?  The window graphs' case: a whole graph on
// one rank, kinds through the hash table with u16 ids, pr_trace = operation_trace, k_tr_a layout.
// Not wide graphs: only pagerank_setup writes their float copies of su (suf).
bool setup_batchable(const mr_graph* g, uint32_t flags) {
    return g->T > 0 && (int64_t)g->T < kind_part_min() && !g->kinds_given && !g->mult.p && g->rs_is_sr && g->rs16.p &&
           g->pr_identity && g->n_pr == g->T && g->fused && !g->wide && g->tperm.p && g->w_tp.p && !g->mw_tp.p &&
           !(flags & MR_PR_EXACT_SUMS) && g->T_all == 0;
}

// pagerank_setup of several graphs (all setup_batchable) in six launches
// keep / dkeep: the descriptors (host and device bytes), owned by the caller until its stream work is done
int pagerank_setup_batch(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, bool fp32,
                         uint64_t seed, uint64_t hmask, std::vector<unsigned char>& keep, DBuf<unsigned char>& dkeep) {
    hipStream_t st = ctx->stream;
    keep.assign((size_t)ng * sizeof(SDev), 0);
    SDev* hs = reinterpret_cast<SDev*>(keep.data());
    int32_t br = 0, bk = 0, bv = 0, bp = 0;
    for (int i = 0; i < ng; ++i) {
        mr_graph* g = gs[i];
        const int32_t N = g->N, T = g->T;
        uint64_t cap = 1;
        while (cap < 2ull * (uint64_t)T) cap <<= 1;
        const int nbp = cdiv(T, TB);   // (n_pr = T)
        MR_TRY(setup_alloc(ctx, g, fp32, true, cap));
        SDev& v = hs[i];
        v.T = T;
        v.N = N;
        v.anomaly = anomaly[i];
        v.fp32 = fp32 ? 1 : 0;
        v.cap = (int64_t)cap;
        v.T_all = T;
        v.cd = (float)(1.0 - d);
        v.phi = g->phi;
        v.pref = g->pref.p;
        v.c_t = g->c_t.p;
        v.c_tp = g->c_tp.p;
        v.tperm = g->tperm.p;
        if (!g->tpos_ok) {   // (graphs prepared one at a time: the inverse of tperm, once per layout)
            MR_TRY(g->tpos.alloc(ctx, (size_t)std::max(T, 1)));
            if (T) hipLaunchKernelGGL(k_inv_perm, dim3(cdiv(T, 256)), dim3(256), 0, st, g->tperm.p, T, g->tpos.p);
            g->tpos_ok = true;
        }
        v.tpos = g->tpos.p;
        v.hk = g->ht_key.p;
        v.cr = g->ht_cr.p;
        v.slot_of = g->slot_of.p;
        v.flag = g->flag.p;
        v.kind = g->kind.p;
        v.scal = g->scal.p;
        v.ppart = g->ppart.p;
        v.w_t = g->w_t.p;
        v.w_tq = g->w_tp.p;
        v.u_o = g->u_o.p;
        v.sp0 = g->spb[0].p;
        v.su0 = g->sub[0].p;
        v.su1 = g->sub[1].p;
        v.q64 = g->q64[0].p;
        v.q32 = g->q32[0].p;
        v.mslot = g->mslot.p;
        v.perm = g->relabeled ? g->perm.p : nullptr;
        v.off = g->rs_off.p;
        v.o16 = g->rs16.p;
        v.len_t = g->len_t.p;
        v.b_reset = br;
        br += reset_grid(T, cap, N);
        v.b_kins = bk;
        bk += cdiv(T, KB);
        v.b_kver = bv;
        bv += cdiv(T, 256);
        v.b_pref = bp;
        bp += nbp;
    }
    MR_TRY(dkeep.upload(ctx, keep.data(), keep.size()));
    const SDev* dsd = reinterpret_cast<const SDev*>(dkeep.p);
    hipLaunchKernelGGL(k_reset_init_b, dim3(br), dim3(256), 0, st, dsd, ng);
    hipLaunchKernelGGL(k_kind_insert_b, dim3(bk), dim3(KB), 0, st, dsd, ng, seed, hmask);
    hipLaunchKernelGGL(k_kind_verify_b, dim3(bv), dim3(256), 0, st, dsd, ng);
    hipLaunchKernelGGL(k_pref_partial_b, dim3(bp), dim3(TB), 0, st, dsd, ng);
    hipLaunchKernelGGL(k_pref_total_b, dim3(ng), dim3(1024), 0, st, dsd);
    hipLaunchKernelGGL(k_pref_apply_b, dim3(bp), dim3(TB), 0, st, dsd, ng);
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;
}

// A graph's kinds, preference and iteration state for its next mr_pagerank(_batch) call with
// these arguments, on THIS context's stream (the one that built it): mr_windows_batch sets up a
// window's graphs while the previous group's iterations run.  The next call on the graph skips
// its own setup when the arguments match (first kind-hash seed; a collision retries in full).
int mr_pagerank_presetup_n(mr_ctx* ctx, mr_graph* const* gs, const int* an, int n, double d, int precision,
                           std::vector<unsigned char>& keep) {
    const bool fp32 = precision == MR_FP32;
    bool batch = n >= 2 && getenv("MR_NO_SETUP_BATCH") == nullptr;
    for (int i = 0; i < n && batch; ++i) batch = gs[i]->N && gs[i]->T && setup_batchable(gs[i], 0);
    if (!batch) {
        for (int i = 0; i < n; ++i) MR_TRY(mr_pagerank_presetup(ctx, gs[i], an[i], d, precision, 0));
        return MR_OK;
    }
    DBuf<unsigned char> dsd;   // (returns to this context's pool: reused only by later work on this stream)
    MR_TRY(pagerank_setup_batch(ctx, gs, an, n, d, fp32, kind_seed(0), kind_hmask(0), keep, dsd));
    for (int i = 0; i < n; ++i) mark_presetup(gs[i], an[i], d, fp32, 0);
    return MR_OK;
}

int mr_pagerank_presetup(mr_ctx* ctx, mr_graph* g, int anomaly, double d, int precision, uint32_t flags) {
    const bool fp32 = precision == MR_FP32;
    if (g->N == 0 || g->T == 0) return MR_OK;   // (the call itself raises)
    MR_TRY(pagerank_setup(ctx, g, anomaly, d, fp32, flags, false, kind_seed(0), kind_hmask(0)));
    mark_presetup(g, anomaly, d, fp32, flags);
    return MR_OK;
}
