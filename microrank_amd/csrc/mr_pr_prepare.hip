// Graph prepare for K2 (mr_graph_prepare, mr_graph_prepare_batch): derived arrays + segments after
// structure upload -- the per-graph constants, the P_sr tiles (compressed sparse blocks) of
// k_iter_a, the op relabelling by coverage (trace_num_list, pagerank.py:98-104), the wide split
// (N > FX_NMAX) and the trace-parallel layout k_tr_a walks.  The iteration itself: mr_pagerank.hip
// (its kernels: mr_pr_walk.hip, mr_pr_fxb.hip, mr_pr_tile_cold.hip; its plan: mr_pr_plan.hip).
#include <algorithm>
#include <cstdlib>

#include "mr_pr_dev.h"
#include "mr_pr_internal.h"
#include "mr_sort.h"

namespace {

constexpr int TSHIFT_MIN = 8, TSHIFT_MAX = 12;   // tiles of 256 .. 4096 traces

// ---------------------------------------------------------------- graph constants
// per-graph constants in one launch: w_t = fp32(1/len_t) (fp64 1/n -> fp32), u_o, pw, and the
// u16 copy of the op ids (N <= 65536)
// (and clears `nz` words of the layout's scratch: tr_layout's histogram and slot counters)
__device__ __forceinline__ void graph_consts_body(int32_t blk, const int32_t* len_t, float* w_t, int32_t T,
                                                  const int32_t* len_o, const int32_t* nchild, float* u_o, float* pw,
                                                  int32_t N, const int32_t* ops, int64_t n, uint16_t* o16,
                                                  int32_t* zero, int32_t nz) {
    const int64_t i = (int64_t)blk * blockDim.x + threadIdx.x;
    if (i < nz) zero[i] = 0;
    if (i < T) w_t[i] = len_t[i] > 0 ? (float)(1.0 / (double)len_t[i]) : 0.0f;
    if (i < N) {
        u_o[i] = len_o[i] > 0 ? (float)(1.0 / (double)len_o[i]) : 0.0f;
        pw[i] = nchild[i] > 0 ? (float)(1.0 / (double)nchild[i]) : 0.0f;
    }
    // the u16 copy, four ids per thread (one 16-B load, one 8-B store instead of 2-B stores)
    if (o16 && 4 * i < n) {
        if (4 * i + 3 < n) {
            const int4 v = *(const int4*)(ops + 4 * i);
            uint2 w;
            w.x = (uint32_t)(uint16_t)v.x | ((uint32_t)(uint16_t)v.y << 16);
            w.y = (uint32_t)(uint16_t)v.z | ((uint32_t)(uint16_t)v.w << 16);
            *(uint2*)(o16 + 4 * i) = w;
        } else {
            for (int64_t k = 4 * i; k < n; ++k) o16[k] = (uint16_t)ops[k];
        }
    }
}
__global__ void k_graph_consts(const int32_t* len_t, float* w_t, int32_t T, const int32_t* len_o, const int32_t* nchild,
                               float* u_o, float* pw, int32_t N, const int32_t* ops, int64_t n, uint16_t* o16,
                               int32_t* zero, int32_t nz) {
    graph_consts_body((int32_t)blockIdx.x, len_t, w_t, T, len_o, nchild, u_o, pw, N, ops, n, o16, zero, nz);
}

// ---------------------------------------------------------------- P_sr tiles (compressed sparse blocks)
// entry (t, o) of the trace-major P_sr incidence -> key (tile(t), o), value t mod tile; a stable
// sort by key leaves every tile's entries in (op, trace) order
__global__ void k_tile_keys(const int64_t* off, const int32_t* ops, int32_t T, int tshift, int nb, uint64_t* key,
                            uint32_t* val) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const uint64_t hi = (uint64_t)(uint32_t)(t >> tshift) << nb;
    const uint32_t lt = (uint32_t)t & ((1u << tshift) - 1u);
    for (int64_t e = off[t]; e < off[t + 1]; ++e) {
        key[e] = hi | (uint32_t)ops[e];
        val[e] = lt;
    }
}
__global__ void k_key_heads(const uint64_t* key, int64_t n, int32_t* head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}
__global__ void k_tile_pairs(const uint64_t* key, const uint32_t* val, const int32_t* head, const int64_t* hpos,
                             int64_t n, int nb, uint16_t* ltr, int32_t* pr_op, int64_t* pr_beg, int32_t* pr_tile) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    ltr[e] = (uint16_t)val[e];
    if (head[e]) {
        const int64_t p = hpos[e];
        const uint64_t k = key[e];
        pr_op[p] = (int32_t)(k & ((1ull << nb) - 1ull));
        pr_beg[p] = e;
        pr_tile[p] = (int32_t)(k >> nb);
    }
    if (e == n - 1) pr_beg[hpos[n]] = n;
}
// out[q] = first i in [0, n) with a[i] >= q (a sorted), q in [0, nq]; n from the device when d_n
template <class K>
__global__ void k_lower_bound(const K* a, int64_t n, const int64_t* d_n, int32_t nq, int32_t* out) {
    const int32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nq) return;
    int64_t lo = 0, hi = d_n ? *d_n : n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)a[mid] < (int64_t)q) lo = mid + 1; else hi = mid;
    }
    out[q] = (int32_t)lo;
}
__global__ void k_pair_op_keys(const int32_t* pr_op, int64_t np, uint64_t* key, uint32_t* val) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    key[p] = (uint64_t)(uint32_t)pr_op[p];
    val[p] = (uint32_t)p;
}
__global__ void k_long_flags(const int64_t* pr_beg, int64_t np, int32_t* flag) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < np) flag[p] = (pr_beg[p + 1] - pr_beg[p]) > LONG_PAIR ? 1 : 0;
}
__global__ void k_long_list(const int32_t* flag, const int64_t* pos, const int32_t* pr_tile, int64_t np, int32_t* lp,
                            int32_t* lp_tile) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np || !flag[p]) return;
    lp[pos[p]] = (int32_t)p;
    lp_tile[pos[p]] = pr_tile[p];
}
__global__ void k_op_pairs(const uint64_t* skey, const uint32_t* sval, int64_t np, int32_t* op_pr, int32_t* op_key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    op_pr[i] = (int32_t)sval[i];
    op_key[i] = (int32_t)skey[i];
}
// coverage = traces containing the op (trace_num_list, pagerank.py:98-104) = its pair lengths
__global__ void k_cov(const int32_t* op_pr_off, const int32_t* op_pr, const int64_t* pr_beg, int32_t N, int32_t* cov) {
    const int32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= N) return;
    int64_t c = 0;
    for (int32_t i = op_pr_off[o]; i < op_pr_off[o + 1]; ++i) c += pr_beg[op_pr[i] + 1] - pr_beg[op_pr[i]];
    cov[o] = (int32_t)c;
}

// fused-path coverage: histogram of the distinct (trace, op) incidence's op ids (N <= FX_NMAX:
// LDS counters per block, one global add per touched op)
__global__ void __launch_bounds__(256) k_cov_hist(const uint16_t* ids, int64_t n, int32_t N, int32_t* cov) {
    extern __shared__ int32_t hcnt[];
    for (int32_t o = threadIdx.x; o < N; o += 256) hcnt[o] = 0;
    __syncthreads();
    const int64_t per = (int64_t)256 * 64;
    const int64_t b0 = (int64_t)blockIdx.x * per;
    for (int64_t e = b0 + threadIdx.x; e < min(b0 + per, n); e += 256) atomicAdd(&hcnt[ids[e]], 1);
    __syncthreads();
    for (int32_t o = threadIdx.x; o < N; o += 256)
        if (hcnt[o]) atomicAdd(&cov[o], hcnt[o]);
}

// ---------------------------------------------------------------- op relabelling (fused, large N)
// ops by descending coverage (ties by op): key = ~cov << 14 | op (N <= 16384)
__global__ void k_relabel_keys(const int32_t* cov, int32_t N, uint64_t* key) {
    const int32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < N) key[o] = ((uint64_t)(~(uint32_t)cov[o]) << 14) | (uint32_t)o;
}
__global__ void k_relabel_perm(const uint64_t* key, int32_t N, int32_t* perm, int32_t* inv) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int32_t o = (int32_t)(key[i] & 0x3fffu);
    perm[i] = o;
    inv[o] = i;
}
__global__ void k_relabel_ids(const uint16_t* ids, int64_t n, const int32_t* inv, uint16_t* out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = (uint16_t)inv[ids[e]];
}

// ---------------------------------------------------------------- wide fused graphs (N > FX_NMAX)
// Ops relabelled by coverage; the WIDE_NA most covered ("hot") ops keep k_tr_a's LDS walk (u16
// ids, su and accumulator in LDS); the other ("cold") entries of each trace are summed per
// position by k_cold_trace and accumulated per op range by k_cold_ops (LDS accumulator of one
// range, (position, op) pairs grouped by range, position order within a range).
constexpr int32_t WIDE_RW_MAX = 19456;  // ops per cold range: k_cold_ops' accumulator <= 152 KB
constexpr int WIDE_CB = 256;            // k_cold_ops blocks over all ranges (one per CU: LDS-bound)
constexpr int32_t WIDE_HIST = 32768;    // coverage counters in LDS (ops above: global adds)
constexpr int WIDE_RMAX = 255;          // ranges (8-bit sort digit)

__global__ void __launch_bounds__(256) k_cov_hist_w(const int32_t* ids, int64_t n, int32_t N, int32_t* cov) {
    extern __shared__ int32_t hcnt[];
    const int32_t NL = min(N, WIDE_HIST);
    for (int32_t o = threadIdx.x; o < NL; o += 256) hcnt[o] = 0;
    __syncthreads();
    const int64_t per = (int64_t)256 * 256;
    const int64_t b0 = (int64_t)blockIdx.x * per;
    for (int64_t e = b0 + threadIdx.x; e < min(b0 + per, n); e += 256) {
        const int32_t o = ids[e];
        if (o < NL) atomicAdd(&hcnt[o], 1);
        else atomicAdd(&cov[o], 1);
    }
    __syncthreads();
    for (int32_t o = threadIdx.x; o < NL; o += 256)
        if (hcnt[o]) atomicAdd(&cov[o], hcnt[o]);
}
// key = ~cov << nbo | op (descending coverage, ties by op)
__global__ void k_relabel_keys_w(const int32_t* cov, int32_t N, int nbo, uint64_t* key) {
    const int32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < N) key[o] = ((uint64_t)(~(uint32_t)cov[o]) << nbo) | (uint32_t)o;
}
__global__ void k_relabel_perm_w(const uint64_t* key, int32_t N, uint64_t omask, int32_t* perm, int32_t* inv) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int32_t o = (int32_t)(key[i] & omask);
    perm[i] = o;
    inv[o] = i;
}
// per trace: hot entries (at least one: a trace without hot ops walks the pad id NA) and cold ones
__global__ void k_wide_count(const int64_t* off, const int32_t* ops, const int32_t* inv, int32_t T, int32_t NA,
                             int32_t* nh, int32_t* nc) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    int32_t h = 0, c = 0;
    for (int64_t e = off[t]; e < off[t + 1]; ++e) {
        if (inv[ops[e]] < NA) ++h;
        else ++c;
    }
    nh[t] = max(h, 1);
    nc[t] = c;
}
__global__ void k_wide_hot(const int64_t* off, const int32_t* ops, const int32_t* inv, int32_t T, int32_t NA,
                           const int64_t* hoff, uint16_t* hot16) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    int64_t k = hoff[t];
    const int64_t k0 = k;
    for (int64_t e = off[t]; e < off[t + 1]; ++e) {
        const int32_t o = inv[ops[e]];
        if (o < NA) hot16[k++] = (uint16_t)o;
    }
    if (k == k0) hot16[k] = (uint16_t)NA;
}
__global__ void k_wide_cold_cnt(const int32_t* tperm, const int32_t* nc, int32_t T, int32_t* cnt) {
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < T) cnt[p] = nc[tperm[p]];
}
// cold entries in position order: op ids for k_cold_trace, and sort keys p << 24 | (op - range
// base) << 8 | range whose one stable 8-bit pass groups them by range (positions stay ascending)
// walked in trace order: thread t reads its own op list (a wave's traces are contiguous in the
// CSR) and writes its cold entries at its position's slots (tpos = inverse of tperm) -- walking
// in position order read a random trace per lane, ~16 lines fetched per trace's 60 B (C5's rank
// share: 21 GB of FETCH_SIZE in one 2.8 ms launch)
__global__ void k_wide_cold_fill_t(const int32_t* tpos, const int64_t* off, const int32_t* ops, const int32_t* inv,
                                   int32_t T, int32_t NA, int32_t RW, const int64_t* coff, int32_t* cops,
                                   uint64_t* key) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int32_t p = tpos[t];
    int64_t k = coff[p];
    for (int64_t e = off[t]; e < off[t + 1]; ++e) {
        const int32_t o = inv[ops[e]];
        if (o < NA) continue;
        const int32_t r = (o - NA) / RW;
        cops[k] = o;
        key[k] = ((uint64_t)p << 24) | ((uint64_t)(o - NA - r * RW) << 8) | (uint64_t)r;
        ++k;
    }
}
// rb[r] = first pair of range r (rb[R] = n)
__global__ void k_wide_bounds(const uint64_t* key, int64_t n, int32_t R, int64_t* rb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t r = (int32_t)(key[i] & 0xff);
    const int32_t rp = i ? (int32_t)(key[i - 1] & 0xff) : -1;
    for (int32_t x = rp + 1; x <= r; ++x) rb[x] = i;
    if (i == n - 1)
        for (int32_t x = r + 1; x <= R; ++x) rb[x] = n;
}
__global__ void k_wide_unpack(const uint64_t* key, int64_t n, int32_t* cp_pos, uint16_t* cp_op) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key[i];
    cp_pos[i] = (int32_t)(k >> 24);
    cp_op[i] = (uint16_t)((k >> 8) & 0xffff);
}
// the widest position span of a k_cold_ops block: an op gets at most that many adds in one row
__global__ void k_wide_span(const int64_t* cb_beg, int32_t n_cb, const int32_t* cp_pos, unsigned long long* span) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_cb) return;
    const int64_t b0 = cb_beg[b], b1 = cb_beg[b + 1];
    if (b1 > b0) atomicMax(span, (unsigned long long)(cp_pos[b1 - 1] - cp_pos[b0] + 1));
}

// Cold entries of the short-tile walk: per wave tile ceil(max cold of its traces / 2) chunks of
// 64 lanes x 2 u32 labels, a lane's entries in cold_ops_p order (k_cold_trace's), pads N + lane
// (a zero su slot).  Secondary sort key of the wide layout (cold count) keeps tiles homogeneous.
__global__ void k_ctile_cnt(const int32_t* coff_p, int32_t T, int32_t W, int32_t* cnt) {
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= W) return;
    int32_t m = 0;
    for (int32_t p = k * WAVE; p < min(k * WAVE + WAVE, T); ++p) m = max(m, coff_p[p + 1] - coff_p[p]);
    cnt[k] = (m + 1) >> 1;
}
__global__ void k_ctile_fill(const int32_t* coff_p, const int32_t* cops, const int64_t* cc64, int32_t T, int32_t N,
                             int32_t W, uint32_t* ctids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)W * WAVE) return;
    const int32_t k = (int32_t)(i / WAVE), lane = (int32_t)(i % WAVE);
    const int32_t p = k * WAVE + lane;
    const int32_t a = p < T ? coff_p[p] : 0, n = p < T ? coff_p[p + 1] - a : 0;
    const int64_t c0 = cc64[k], nc = cc64[k + 1] - c0;
    for (int64_t c = 0; c < nc; ++c)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t e = 2 * c + q;
            ctids[((size_t)(c0 + c) * WAVE + lane) * 2 + q] = e < n ? (uint32_t)cops[a + e] : (uint32_t)(N + lane);
        }
}
// sort keys of a layout with a secondary key: (length << 4 | min(skey, 15)), the trace as value
__global__ void k_tr_skey(const int64_t* off, const int32_t* skey, int32_t T, uint64_t* key, uint32_t* val) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    key[t] = ((uint64_t)(off[t + 1] - off[t]) << 4) | (uint64_t)(skey ? min(skey[t], 15) : 0);
    val[t] = (uint32_t)t;
}
__global__ void k_tr_perm_w(const uint32_t* val, const float* w_t, int32_t T, int32_t* tperm, float* w_tp) {
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= T) return;
    const int32_t t = (int32_t)val[p];
    tperm[p] = t;
    w_tp[p] = w_t[t];
}

// ---------------------------------------------------------------- trace-parallel layout (k_tr_a)
// Traces by op count: a counting sort (lengths <= N <= FX_NMAX), order within a length free --
// nothing numeric depends on it (a trace's ids are rotated by trace mod len, not by position;
// the accumulator is integer).  Blocks of TRB threads take TRB * TR_PER traces each: 16 per
// thread for large graphs, 2 for window-sized ones (187k traces in 12 blocks had left the chip idle)
constexpr int TRB = 1024, TR_PER_BIG = 16, TR_PER_SMALL = 2;
template <int TR_PER>
__device__ __forceinline__ void tr_hist_body(int32_t blk, const int64_t* off, int32_t T, int32_t nbin, int32_t* hist) {
    extern __shared__ int32_t lh[];
    for (int32_t i = threadIdx.x; i < nbin; i += TRB) lh[i] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blk * TRB * TR_PER;
    for (int32_t j = 0; j < TR_PER; ++j) {
        const int64_t t = t0 + (int64_t)j * TRB + threadIdx.x;
        if (t < T) atomicAdd(&lh[off[t + 1] - off[t]], 1);
    }
    __syncthreads();
    for (int32_t i = threadIdx.x; i < nbin; i += TRB)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}
template <int TR_PER>
__global__ void __launch_bounds__(TRB) k_tr_hist(const int64_t* off, int32_t T, int32_t nbin, int32_t* hist) {
    tr_hist_body<TR_PER>((int32_t)blockIdx.x, off, T, nbin, hist);
}
// positions: bin start (cursor, claimed per block and bin) + the trace's rank in its block's bin
// A bin's slots: boff given -- its start plus the bin's remaining count, handed out from the end
// (hist is consumed, no cursor copy); boff null (nbin <= TP_LSCAN) -- each block scans the
// histogram in LDS itself and claims slots through `taken` (no scan launch)
constexpr int TP_LSCAN = 8192;
template <int TR_PER>
__device__ __forceinline__ void tr_place_body(int32_t blk, const int64_t* off, int32_t T, int32_t nbin,
                                              const int64_t* boff, int32_t* hist, int32_t* taken, const float* w_t,
                                              int32_t* tperm, float* w_tp, int32_t* tpos) {
    extern __shared__ int32_t lh[];
    int32_t* lbase = lh + nbin;
    for (int32_t i = threadIdx.x; i < nbin; i += TRB) lh[i] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blk * TRB * TR_PER;
    int32_t rk[TR_PER], ln[TR_PER];
#pragma unroll
    for (int32_t j = 0; j < TR_PER; ++j) {
        const int64_t t = t0 + (int64_t)j * TRB + threadIdx.x;
        ln[j] = t < T ? (int32_t)(off[t + 1] - off[t]) : -1;
        rk[j] = ln[j] >= 0 ? atomicAdd(&lh[ln[j]], 1) : 0;
    }
    __syncthreads();
    if (boff) {
        for (int32_t i = threadIdx.x; i < nbin; i += TRB)
            if (lh[i]) lbase[i] = (int32_t)boff[i] + atomicSub(&hist[i], lh[i]) - lh[i];
    } else {
        __shared__ int32_t sbuf[TRB];
        const int32_t per = (nbin + TRB - 1) / TRB, b0 = threadIdx.x * per, b1 = min(b0 + per, nbin);
        int32_t run = 0;
        for (int32_t i = b0; i < b1; ++i) run += hist[i];
        sbuf[threadIdx.x] = run;
        __syncthreads();
        for (int o = 1; o < TRB; o <<= 1) {
            const int32_t v = threadIdx.x >= o ? sbuf[threadIdx.x - o] : 0;
            __syncthreads();
            sbuf[threadIdx.x] += v;
            __syncthreads();
        }
        run = sbuf[threadIdx.x] - run;   // exclusive start of this thread's bins
        for (int32_t i = b0; i < b1; ++i) {
            const int32_t c = hist[i];
            lbase[i] = run + (lh[i] ? atomicAdd(&taken[i], lh[i]) : 0);
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int32_t j = 0; j < TR_PER; ++j) {
        if (ln[j] < 0) continue;
        const int32_t t = (int32_t)(t0 + (int64_t)j * TRB + threadIdx.x);
        const int32_t p = lbase[ln[j]] + rk[j];
        tperm[p] = t;
        w_tp[p] = w_t[t];
        if (tpos) tpos[t] = p;   // (the inverse, stored in trace order)
    }
}
template <int TR_PER>
__global__ void __launch_bounds__(TRB) k_tr_place(const int64_t* off, int32_t T, int32_t nbin, const int64_t* boff,
                                                  int32_t* hist, int32_t* taken, const float* w_t, int32_t* tperm,
                                                  float* w_tp) {
    tr_place_body<TR_PER>((int32_t)blockIdx.x, off, T, nbin, boff, hist, taken, w_t, tperm, w_tp, nullptr);
}
__global__ void __launch_bounds__(TS_T) k_tr_chunk_scan(const int32_t* tperm, const int64_t* off, int32_t T, int32_t n_wt,
                                                        int64_t* c64, int32_t* coff, unsigned long long* st,
                                                        uint64_t epoch) {
    tr_chunk_scan_body((int32_t)blockIdx.x, (int32_t)gridDim.x, tperm, off, T, n_wt, c64, coff, st, epoch);
}
__global__ void k_tr_coff(const int64_t* c64, int32_t n, int32_t* coff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) coff[i] = (int32_t)c64[i];
}
// thread per (tile, lane): the lane's trace rotated by (trace mod len), then pads N + lane
__device__ __forceinline__ void tr_fill_body(int32_t blk, const int32_t* tperm, const int64_t* off, const uint16_t* ids,
                                             const int64_t* c64, int32_t T, int32_t N, int32_t n_wt, uint16_t* tids) {
    const int64_t i = (int64_t)blk * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_wt * WAVE) return;
    const int32_t k = (int32_t)(i / WAVE), lane = (int32_t)(i % WAVE);
    const int64_t p = (int64_t)k * WAVE + lane;
    int64_t a = 0, len = 0, rot = 0;
    if (p < T) {
        const int32_t t = tperm[p];
        a = off[t];
        len = off[t + 1] - a;
        rot = len ? t % len : 0;
    }
    const int64_t nc = c64[k + 1] - c64[k];
    unsigned long long* dst = (unsigned long long*)tids + (size_t)c64[k] * WAVE + lane;   // 4 ids per 8-B store
    // the ids from the rotation start, padded with N + lane; TF_CH chunks per round, their loads
    // issued together (id e of the rotation sits at (rot + e) mod len: no carried index), so a
    // window trace of <= 16 ids costs one load latency instead of one per chunk
    constexpr int TF_CH = 4;
    for (int64_t c0 = 0; c0 < nc; c0 += TF_CH) {
        uint16_t idv[4 * TF_CH];
#pragma unroll
        for (int q = 0; q < 4 * TF_CH; ++q) {
            const int64_t e = 4 * c0 + q, jx = rot + e;
            idv[q] = e < len ? ids[a + (jx >= len ? jx - len : jx)] : (uint16_t)(N + lane);
        }
#pragma unroll
        for (int u = 0; u < TF_CH; ++u)
            if (c0 + u < nc)
                dst[(size_t)(c0 + u) * WAVE] = (unsigned long long)idv[4 * u] | (unsigned long long)idv[4 * u + 1] << 16 |
                                               (unsigned long long)idv[4 * u + 2] << 32 |
                                               (unsigned long long)idv[4 * u + 3] << 48;
    }
}
__global__ void k_tr_fill(const int32_t* tperm, const int64_t* off, const uint16_t* ids, const int64_t* c64, int32_t T,
                          int32_t N, int32_t n_wt, uint16_t* tids) {
    tr_fill_body((int32_t)blockIdx.x, tperm, off, ids, c64, T, N, n_wt, tids);
}
// Register-accumulated hot ops (large graphs): the HOT_MAX ops present in the most traces leave the
// id chunks -- op 0 of the C4 graph is in every trace, so each 16-lane atomic group of every step
// that holds it adds to ONE LDS address 16 times -- and trace t keeps the bit set of the hot ops it
// holds instead (hmask).  A trace whose ops are all hot keeps its first one in the list (no empty
// traces: every tile has a chunk).  hidx[o] = h or -1.
__global__ void __launch_bounds__(256) k_hot_count(const int64_t* off, const uint16_t* ids, int32_t T, const int8_t* hidx,
                                                   int32_t N, int32_t* rlen, uint8_t* mask) {
    extern __shared__ int8_t lh8[];
    for (int32_t o = threadIdx.x; o < N; o += 256) lh8[o] = hidx[o];
    __syncthreads();
    const int32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    uint32_t m = 0, first = 0xffu;
    int32_t n = 0;
    for (int64_t e = off[t]; e < off[t + 1]; ++e) {
        const int h = lh8[ids[e]];
        if (h >= 0) {
            if (first == 0xffu) first = (uint32_t)h;
            m |= 1u << h;
        } else {
            ++n;
        }
    }
    if (n == 0 && m) {   // all hot: the first stays in the list
        m &= ~(1u << first);
        n = 1;
    }
    rlen[t] = n;
    mask[t] = (uint8_t)m;
}
__global__ void __launch_bounds__(256) k_hot_fill(const int64_t* off, const uint16_t* ids, int32_t T, const int8_t* hidx,
                                                  int32_t N, const uint8_t* mask, const int64_t* roff, uint16_t* rids) {
    extern __shared__ int8_t lh8[];
    for (int32_t o = threadIdx.x; o < N; o += 256) lh8[o] = hidx[o];
    __syncthreads();
    const int32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const uint32_t m = mask[t];
    int64_t w = roff[t];
    for (int64_t e = off[t]; e < off[t + 1]; ++e) {
        const uint16_t o = ids[e];
        const int h = lh8[o];
        if (h < 0 || !((m >> h) & 1u)) rids[w++] = o;
    }
}
__global__ void k_hot_perm(const int32_t* tperm, const uint8_t* mask, int32_t T, uint8_t* hmask) {
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < T) hmask[p] = mask[tperm[p]];
}

constexpr int64_t TR_LARGE = (int64_t)1 << 20;   // "large graph": the hot-op threshold

// The prepare of several small fused graphs (a window's two) in one launch per step: block ranges
// per graph, the same bodies (mr_graph_prepare_batch)
struct PDev {
    int32_t T, N, nbin, W, nz, n_cs;
    int64_t nnz, st_off;
    int32_t b_gc, b_th, b_cs, b_fill;
    const int32_t *len_t, *len_o, *nchild, *rs_ops;
    const int64_t* rs_off;
    float *w_t, *u_o, *pw, *w_tp;
    uint16_t *rs16, *tids;
    int32_t *trz, *tperm, *coff, *tpos;
    int64_t* c64;
};
__global__ void k_graph_consts_b(const PDev* __restrict__ pd, int32_t n) {
    const PDev& G = pd[block_owner<PDev, &PDev::b_gc>(pd, n, (int32_t)blockIdx.x)];
    graph_consts_body((int32_t)blockIdx.x - G.b_gc, G.len_t, G.w_t, G.T, G.len_o, G.nchild, G.u_o, G.pw, G.N, G.rs_ops,
                      G.nnz, G.rs16, G.trz, G.nz);
}
__global__ void __launch_bounds__(TRB) k_tr_hist_b(const PDev* __restrict__ pd, int32_t n) {
    const PDev& G = pd[block_owner<PDev, &PDev::b_th>(pd, n, (int32_t)blockIdx.x)];
    tr_hist_body<TR_PER_SMALL>((int32_t)blockIdx.x - G.b_th, G.rs_off, G.T, G.nbin, G.trz);
}
__global__ void __launch_bounds__(TRB) k_tr_place_b(const PDev* __restrict__ pd, int32_t n) {
    const PDev& G = pd[block_owner<PDev, &PDev::b_th>(pd, n, (int32_t)blockIdx.x)];
    tr_place_body<TR_PER_SMALL>((int32_t)blockIdx.x - G.b_th, G.rs_off, G.T, G.nbin, nullptr, G.trz, G.trz + G.nbin,
                                G.w_t, G.tperm, G.w_tp, G.tpos);
}
__global__ void __launch_bounds__(TS_T) k_tr_chunk_scan_b(const PDev* __restrict__ pd, int32_t n, unsigned long long* st,
                                                         uint64_t epoch) {
    const PDev& G = pd[block_owner<PDev, &PDev::b_cs>(pd, n, (int32_t)blockIdx.x)];
    tr_chunk_scan_body((int32_t)blockIdx.x - G.b_cs, G.n_cs, G.tperm, G.rs_off, G.T, G.W, G.c64, G.coff, st + G.st_off,
                       epoch);
}
__global__ void k_tr_fill_b(const PDev* __restrict__ pd, int32_t n) {
    const PDev& G = pd[block_owner<PDev, &PDev::b_fill>(pd, n, (int32_t)blockIdx.x)];
    tr_fill_body((int32_t)blockIdx.x - G.b_fill, G.tperm, G.rs_off, G.rs16, G.c64, G.T, G.N, G.W, G.tids);
}

}  // namespace

// k_tr_a's layout of a fused graph (after w_t and the kernel's ids rs16 / rsp): traces sorted by
// op count, tiles of 64 positions, ids lane-interleaved in chunks of 4.  One host round trip (the
// chunk count sizes the id array; the chunk offsets stay on the host for the per-wave cut).
// off / ids: the trace-major incidence the kernel walks (rs_off with rs16 / rsp, or a wide graph's
// hot entries), N: the kernel's op count (pads N + lane)
// hot ops stripped from the id chunks (register-accumulated in k_tr_a): MR_TR_HOT ops (default
// HOT_MAX, 0 = none) covering at least 1/8 of the traces, on graphs of >= MR_TR_HOT_MIN traces
// (default 2^20: window graphs keep their layout) whose su fits in LDS
static int hot_strip(mr_ctx* ctx, mr_graph* g, const int64_t*& off, const uint16_t*& src, int32_t N, int64_t& nent,
                     DBuf<int64_t>& roff, DBuf<uint16_t>& rids, DBuf<uint8_t>& mask) {
    // (read per preparation: tests flip them)
    const char* eh = getenv("MR_TR_HOT");
    const char* em = getenv("MR_TR_HOT_MIN");
    const int hcap = g->wide ? HOT_MAX_WIDE : HOT_MAX;   // (the wide variant carries fewer accumulators)
    const int hmax = eh ? std::min(std::max(atoi(eh), 0), hcap) : hcap;
    const int64_t tmin = em ? (int64_t)atoll(em) : TR_LARGE;
    g->nhr = 0;
    g->hmask.reset();
    const int32_t T = g->T;
    if (hmax == 0 || (int64_t)T < tmin || N < 1 || N > 16384 || !tr_hot_fits(N)) return MR_OK;
    hipStream_t st = ctx->stream;
    std::vector<int32_t> cov((size_t)N);
    if (!g->wide && g->cov.p) {   // the kernel's ids are the graph's: its coverage (prepare / build) serves
        MR_TRY(g->cov.download(ctx, cov.data(), (size_t)N));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    } else {   // (wide graphs: the hot half's relabelled ids)
        DBuf<int32_t> dc;
        MR_TRY(dc.zero(ctx, (size_t)N));
        if (nent)
            hipLaunchKernelGGL(k_cov_hist, dim3(cdiv(nent, 256 * 64)), dim3(256), (size_t)N * sizeof(int32_t), st, src,
                               nent, N, dc.p);
        MR_TRY(dc.download(ctx, cov.data(), (size_t)N));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    }
    std::vector<int32_t> ord((size_t)N);
    for (int32_t o = 0; o < N; ++o) ord[(size_t)o] = o;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return cov[(size_t)a] > cov[(size_t)b]; });
    std::vector<int8_t> hidx((size_t)N, (int8_t)-1);
    int nh = 0;
    for (; nh < hmax && nh < N && (int64_t)cov[(size_t)ord[(size_t)nh]] * 8 >= (int64_t)T; ++nh) {
        hidx[(size_t)ord[(size_t)nh]] = (int8_t)nh;
        g->hop[nh] = ord[(size_t)nh];
    }
    // worth its pass only when the hot ops carry a quarter of the entries: the C4 graph's top 8
    // carry 26 % (iteration 154 -> 145 us); the span-built C4 graph's 23 % (op 0 in every trace, then
    // seven at 30 %) gained nothing measurable per iteration while the strip added ~1 ms to its
    // build (c4 --from-spans, A/B in the commit log)
    // (MR_TR_HOT_FRAC: that share, default 0.25; tests force the layout with 0)
    const char* ef = getenv("MR_TR_HOT_FRAC");
    const double fmin = ef ? atof(ef) : 0.25;
    int64_t hsum = 0;
    for (int h = 0; h < nh; ++h) hsum += cov[(size_t)g->hop[h]];
    if (nh == 0 || (double)hsum < fmin * (double)nent) return MR_OK;
    DBuf<int8_t> dh;
    DBuf<int32_t> rlen;
    DBuf<int64_t> tmp;
    MR_TRY(dh.upload(ctx, hidx.data(), hidx.size()));
    MR_TRY(rlen.alloc(ctx, (size_t)T));
    MR_TRY(mask.alloc(ctx, (size_t)T));
    MR_TRY(roff.alloc(ctx, (size_t)T + 1));
    MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(T)));
    hipLaunchKernelGGL(k_hot_count, dim3(cdiv(T, 256)), dim3(256), (size_t)N, st, off, src, T, dh.p, N, rlen.p, mask.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, rlen.p, roff.p, T, tmp.p));
    // (sized by the full entry count: no read-back; nent stays an upper bound for the layout)
    MR_TRY(rids.alloc(ctx, (size_t)std::max<int64_t>(nent, 1) + 8));
    hipLaunchKernelGGL(k_hot_fill, dim3(cdiv(T, 256)), dim3(256), (size_t)N, st, off, src, T, dh.p, N, mask.p, roff.p, rids.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (the host hidx leaves scope)
    g->nhr = nh;
    off = roff.p;
    src = rids.p;
    return MR_OK;
}

static int tr_layout(mr_ctx* ctx, mr_graph* g, const int64_t* off, const uint16_t* src, int32_t N, int64_t nent,
                     int32_t* zeroed, const int32_t* skey = nullptr) {
    hipStream_t st = ctx->stream;
    const int32_t T = g->T;
    DBuf<int64_t> roff;
    DBuf<uint16_t> rids;
    DBuf<uint8_t> hm;
    MR_TRY(hot_strip(ctx, g, off, src, N, nent, roff, rids, hm));
    const int32_t W = cdiv(T, WAVE);
    g->n_wt = W;
    g->wtile_nw = 0;
    const int32_t nbin = N + 1;   // trace lengths 1..N (distinct ops)
    // zeroed: 2 * nbin words the caller cleared (histogram, slot counters), else cleared here
    const bool lscan = nbin <= TP_LSCAN;
    DBuf<int32_t> hz;
    DBuf<int64_t> boff, c64, tmp;
    if (!zeroed) {
        MR_TRY(hz.zero(ctx, 2 * (size_t)nbin));
        zeroed = hz.p;
    }
    int32_t* hist = zeroed;
    int32_t* taken = zeroed + nbin;
    MR_TRY(c64.alloc(ctx, (size_t)W + 1));
    MR_TRY(g->tperm.alloc(ctx, (size_t)std::max(T, 1)));
    MR_TRY(g->w_tp.alloc(ctx, (size_t)std::max(T, 1)));
    g->tpos_ok = false;
    MR_TRY(g->coff.alloc(ctx, (size_t)W + 1));
    // (length, secondary key): a stable radix sort, equal keys in trace order -- for wide graphs (the
    // cold count as secondary key) and kind-compressed ones, whose fixed-point scale depends on
    // the tiles' multiplicity sums (the counting sort below orders equal lengths run-dependently)
    if (T && (skey || g->kinds_given)) {
        DBuf<uint64_t> key;
        DBuf<uint32_t> val;
        MR_TRY(key.alloc(ctx, (size_t)T));
        MR_TRY(val.alloc(ctx, (size_t)T));
        hipLaunchKernelGGL(k_tr_skey, dim3(cdiv(T, 256)), dim3(256), 0, st, off, skey, T, key.p, val.p);
        {
            SortScratch ws;
            MR_TRY(mr_radix_sort(ctx, key.p, val.p, T, bits_for((uint64_t)N) + 4, ws));
        }
        hipLaunchKernelGGL(k_tr_perm_w, dim3(cdiv(T, 256)), dim3(256), 0, st, val.p, g->w_t.p, T, g->tperm.p, g->w_tp.p);
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    } else if (T) {
        const bool big = (int64_t)T >= (int64_t)num_cus() * TRB * TR_PER_SMALL * 4;
        const int per = big ? TR_PER_BIG : TR_PER_SMALL;
        const int nb = cdiv(T, (int64_t)TRB * per);
        hipLaunchKernelGGL(big ? k_tr_hist<TR_PER_BIG> : k_tr_hist<TR_PER_SMALL>, dim3(nb), dim3(TRB),
                           (size_t)nbin * sizeof(int32_t), st, off, T, nbin, hist);
        if (!lscan) {
            MR_TRY(boff.alloc(ctx, (size_t)nbin + 1));
            MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(nbin)));
            MR_TRY(mr_exclusive_scan_i32(ctx, hist, boff.p, nbin, tmp.p));
        }
        hipLaunchKernelGGL(big ? k_tr_place<TR_PER_BIG> : k_tr_place<TR_PER_SMALL>, dim3(nb), dim3(TRB),
                           2 * (size_t)nbin * sizeof(int32_t), st, off, T, nbin,
                           lscan ? (const int64_t*)nullptr : boff.p, hist, taken, g->w_t.p, g->tperm.p, g->w_tp.p);
    }
    {   // chunk counts per wave tile, their prefix and its int32 copy: one launch
        const int64_t nt = std::max<int64_t>(cdiv((int64_t)W, TS_TILE), 1);
        unsigned long long* dst = nullptr;
        uint64_t epoch = 0;
        MR_TRY(mr_dl_status(ctx, nt, &dst, &epoch));
        hipLaunchKernelGGL(k_tr_chunk_scan, dim3((unsigned)nt), dim3(TS_T), 0, st, g->tperm.p, off, T, W, c64.p,
                           g->coff.p, dst, epoch);
    }
    // the id array at an upper bound of the chunk count (no host round trip): tile k holds
    // ceil(maxlen_k / 4) chunks, and with lengths ascending maxlen_k <= every
    // length of tile k + 1, so sum_k maxlen_k <= nent / 64 + 2 N
    g->coff_h.clear();
    const int64_t nch = 2 * (int64_t)W + (nent / WAVE + 2 * (int64_t)N) / 4 + 2;
    MR_TRY(g->tids.alloc(ctx, (size_t)std::max<int64_t>(nch, 1) * WAVE * 4));
    if (W)
        hipLaunchKernelGGL(k_tr_fill, dim3(cdiv((int64_t)W * WAVE, 256)), dim3(256), 0, st, g->tperm.p, off, src,
                           c64.p, T, N, W, g->tids.p);
    if (g->nhr) {   // the hot-op bits in position order
        MR_TRY(g->hmask.alloc(ctx, (size_t)T));
        hipLaunchKernelGGL(k_hot_perm, dim3(cdiv(T, 256)), dim3(256), 0, st, g->tperm.p, hm.p, T, g->hmask.p);
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (the stripped lists leave scope)
    }
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;   // (scratch returns to the stream-ordered pool)
}

// A wide fused graph (N > FX_NMAX): ops relabelled by coverage, hot entries (labels < NA) laid
// out for k_tr_a, cold entries per position for k_cold_trace and grouped by op range for
// k_cold_ops with the blocks of each range (about WIDE_CB over all ranges, by pair count).
static int wide_prepare(mr_ctx* ctx, mr_graph* g) {
    hipStream_t st = ctx->stream;
    const int32_t N = g->N, T = g->T, NA = WIDE_NA;
    const int64_t nnz = g->nnz_sr;
    g->wide = true;
    g->NA = NA;
    g->rsp.reset();
    // ---- coverage, then labels by descending coverage (perm[new] = old)
    if (!g->cov_ready) MR_TRY_HIP(ctx, hipMemsetAsync(g->cov.p, 0, (size_t)N * sizeof(int32_t), st));
    if (nnz && !g->cov_ready)
        hipLaunchKernelGGL(k_cov_hist_w, dim3(cdiv(nnz, (int64_t)256 * 256)), dim3(256),
                           (size_t)std::min(N, WIDE_HIST) * sizeof(int32_t), st, g->rs_ops.p, nnz, N, g->cov.p);
    const int nbo = bits_for((uint64_t)(N - 1));
    DBuf<uint64_t> key;
    DBuf<int32_t> inv;
    MR_TRY(key.alloc(ctx, (size_t)N));
    MR_TRY(inv.alloc(ctx, (size_t)N));
    MR_TRY(g->perm.alloc(ctx, (size_t)N));
    hipLaunchKernelGGL(k_relabel_keys_w, dim3(cdiv(N, 256)), dim3(256), 0, st, g->cov.p, N, nbo, key.p);
    {
        SortScratch ws;
        MR_TRY(mr_radix_sort(ctx, key.p, nullptr, N, nbo + 32, ws));
    }
    hipLaunchKernelGGL(k_relabel_perm_w, dim3(cdiv(N, 256)), dim3(256), 0, st, key.p, N, (1ull << nbo) - 1ull, g->perm.p,
                       inv.p);
    g->relabeled = true;
    // ---- hot entries per trace (u16, node order; a trace without any walks the pad id NA)
    DBuf<int32_t> nh, nc;
    DBuf<int64_t> tmp;
    MR_TRY(nh.alloc(ctx, (size_t)T));
    MR_TRY(nc.alloc(ctx, (size_t)T));
    MR_TRY(g->hot_off.alloc(ctx, (size_t)T + 1));
    MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(std::max<int64_t>(T, 1))));
    hipLaunchKernelGGL(k_wide_count, dim3(cdiv(T, 256)), dim3(256), 0, st, g->rs_off.p, g->rs_ops.p, inv.p, T, NA, nh.p,
                       nc.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, nh.p, g->hot_off.p, T, tmp.p));
    int64_t n_hot = 0;
    MR_TRY_HIP(ctx, hipMemcpyAsync(&n_hot, g->hot_off.p + T, sizeof n_hot, hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    MR_TRY(g->hot16.alloc(ctx, (size_t)n_hot + 8));
    hipLaunchKernelGGL(k_wide_hot, dim3(cdiv(T, 256)), dim3(256), 0, st, g->rs_off.p, g->rs_ops.p, inv.p, T, NA,
                       g->hot_off.p, g->hot16.p);
    MR_TRY(tr_layout(ctx, g, g->hot_off.p, g->hot16.p, NA, n_hot, nullptr, nc.p));   // tperm, w_tp, tids, coff
    // ---- cold entries in position order
    DBuf<int32_t> cnt;
    DBuf<int64_t> coff64;
    MR_TRY(cnt.alloc(ctx, (size_t)T));
    MR_TRY(coff64.alloc(ctx, (size_t)T + 1));
    hipLaunchKernelGGL(k_wide_cold_cnt, dim3(cdiv(T, 256)), dim3(256), 0, st, g->tperm.p, nc.p, T, cnt.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, cnt.p, coff64.p, T, tmp.p));
    int64_t n_cold = 0;
    MR_TRY_HIP(ctx, hipMemcpyAsync(&n_cold, coff64.p + T, sizeof n_cold, hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    g->n_cold = n_cold;
    MR_TRY(g->cold_off_p.alloc(ctx, (size_t)T + 1));
    hipLaunchKernelGGL(k_tr_coff, dim3(cdiv((int64_t)T + 1, 256)), dim3(256), 0, st, coff64.p, T, g->cold_off_p.p);
    const int32_t W = g->n_wt;
    // ---- cold tiles of the short-tile walk (after cold_ops_p, below) and the long-tile start
    DBuf<int32_t> ccnt;
    DBuf<int64_t> cc64;
    MR_TRY(ccnt.alloc(ctx, (size_t)std::max(W, 1)));
    MR_TRY(cc64.alloc(ctx, (size_t)W + 1));
    MR_TRY(g->ccoff.alloc(ctx, (size_t)W + 1));
    const int32_t R = (int32_t)cdiv((int64_t)N - NA, WIDE_RW_MAX);
    const int32_t RW = (int32_t)(cdiv(cdiv((int64_t)N - NA, R), WAVE) * WAVE);
    g->n_ranges = R;
    g->cold_rw = RW;
    MR_TRY(g->cold_ops_p.alloc(ctx, (size_t)n_cold + 1));
    MR_TRY(g->cp_pos.alloc(ctx, (size_t)n_cold + 1));
    MR_TRY(g->cp_op.alloc(ctx, (size_t)n_cold + 1));
    DBuf<int64_t> rb;
    MR_TRY(rb.zero(ctx, (size_t)R + 1));
    {
        DBuf<uint64_t> ck;
        MR_TRY(ck.alloc(ctx, (size_t)n_cold + 1));
        if (T && !g->tpos_ok) {   // (the inverse of this layout's tperm; the preference reuses it)
            MR_TRY(g->tpos.alloc(ctx, (size_t)T));
            inv_perm_launch(ctx, g->tperm.p, T, g->tpos.p);
            g->tpos_ok = true;
        }
        if (T)
            hipLaunchKernelGGL(k_wide_cold_fill_t, dim3(cdiv(T, 256)), dim3(256), 0, st, g->tpos.p, g->rs_off.p,
                               g->rs_ops.p, inv.p, T, NA, RW, coff64.p, g->cold_ops_p.p, ck.p);
        SortScratch ws;
        MR_TRY(mr_radix_sort(ctx, ck.p, nullptr, n_cold, 8, ws));   // stable: positions stay ascending
        if (n_cold) {
            hipLaunchKernelGGL(k_wide_bounds, dim3(cdiv(n_cold, 256)), dim3(256), 0, st, ck.p, n_cold, R, rb.p);
            hipLaunchKernelGGL(k_wide_unpack, dim3(cdiv(n_cold, 256)), dim3(256), 0, st, ck.p, n_cold, g->cp_pos.p,
                               g->cp_op.p);
        }
    }
    if (W) {
        hipLaunchKernelGGL(k_ctile_cnt, dim3(cdiv(W, 256)), dim3(256), 0, st, g->cold_off_p.p, T, W, ccnt.p);
        DBuf<int64_t> tmp2;
        MR_TRY(tmp2.alloc(ctx, (size_t)scan_tmp_elems(W)));
        MR_TRY(mr_exclusive_scan_i32(ctx, ccnt.p, cc64.p, W, tmp2.p));
        hipLaunchKernelGGL(k_tr_coff, dim3(cdiv((int64_t)W + 1, 256)), dim3(256), 0, st, cc64.p, W, g->ccoff.p);
        int64_t nch = 0;
        MR_TRY_HIP(ctx, hipMemcpyAsync(&nch, cc64.p + W, sizeof nch, hipMemcpyDeviceToHost, st));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
        MR_TRY(g->ctids.alloc(ctx, (size_t)std::max<int64_t>(nch, 1) * WAVE * 2));
        hipLaunchKernelGGL(k_ctile_fill, dim3(cdiv((int64_t)W * WAVE, 256)), dim3(256), 0, st, g->cold_off_p.p,
                           g->cold_ops_p.p, cc64.p, T, N, W, g->ctids.p);
        // long tiles (more hot chunks than the short walk's last tier) and short tiles with more
        // than two cold chunks keep k_cold_trace's sums: the list of those tiles
        std::vector<int32_t> co((size_t)W + 1), cn((size_t)W), tl;
        MR_TRY(g->coff.download(ctx, co.data(), co.size()));
        MR_TRY(ccnt.download(ctx, cn.data(), cn.size()));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
        for (int32_t k = 0; k < W; ++k)
            if (co[(size_t)k + 1] - co[(size_t)k] > std::min(TR_TIERS_EXT, TR_TIERS_W32) || cn[(size_t)k] > 2) tl.push_back(k);
        g->n_ctl = (int32_t)tl.size();
        MR_TRY(g->ctl.alloc(ctx, std::max<size_t>(tl.size(), 1)));
        if (!tl.empty()) MR_TRY(g->ctl.upload(ctx, tl.data(), tl.size()));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (the host list leaves scope)
    } else {
        MR_TRY_HIP(ctx, hipMemsetAsync(g->ccoff.p, 0, sizeof(int32_t), st));
        g->n_ctl = 0;
    }
    std::vector<int64_t> rbh((size_t)R + 1);
    MR_TRY(rb.download(ctx, rbh.data(), rbh.size()));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    // ---- k_cold_ops blocks: each range's pairs in equal slices, blocks proportional to its pairs
    std::vector<int32_t> rowbase((size_t)R + 1);
    std::vector<int64_t> beg;
    for (int32_t r = 0; r < R; ++r) {
        const int64_t pr = rbh[(size_t)r + 1] - rbh[(size_t)r];
        const int64_t nbr = std::max<int64_t>(1, (int64_t)std::llround((double)WIDE_CB * (double)pr / (double)std::max<int64_t>(n_cold, 1)));
        rowbase[(size_t)r] = (int32_t)beg.size();
        for (int64_t j = 0; j < nbr; ++j) beg.push_back(rbh[(size_t)r] + pr * j / nbr);
    }
    rowbase[(size_t)R] = (int32_t)beg.size();
    beg.push_back(rbh[(size_t)R]);
    g->n_cb = (int32_t)beg.size() - 1;
    MR_TRY(g->cb_beg.upload(ctx, beg.data(), beg.size()));
    MR_TRY(g->cold_rowbase.upload(ctx, rowbase.data(), rowbase.size()));
    MR_TRY(g->cold_part.alloc(ctx, (size_t)g->n_cb * (size_t)RW));
    MR_TRY(g->cold_acc.alloc(ctx, (size_t)T));
    DBuf<unsigned long long> span;
    MR_TRY(span.zero(ctx, 1));
    hipLaunchKernelGGL(k_wide_span, dim3(cdiv(g->n_cb, 256)), dim3(256), 0, st, g->cb_beg.p, g->n_cb, g->cp_pos.p, span.p);
    unsigned long long sp = 0;
    MR_TRY(span.download(ctx, &sp, 1));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (also: the host vectors leave scope)
    g->cold_span = std::max<uint64_t>(sp, 1);
    g->n_tiles = 0;
    g->n_pairs = 0;
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;
}

// Derived per-graph arrays: fp32 reciprocals, u16 ids, and the P_sr tiles.  One host round trip
// (the number of (tile, op) pairs sizes the pair arrays).
// mr_graph_prepare of several graphs built from spans (a window's two): one launch per step when
// all are small fused graphs whose su stays in LDS (no relabelling, one-block histogram scan),
// else one prepare each.  keep: the descriptors' host copy, alive until the stream has used it.
int mr_graph_prepare_batch(mr_ctx* ctx, mr_graph* const* gs, int n, std::vector<unsigned char>& keep) {
    const bool off = getenv("MR_NO_PREP_BATCH") != nullptr;   // A/B knob (read per call: tests flip it)
    bool ok = !off && n >= 2 && getenv("MR_NO_FUSED") == nullptr;
    for (int i = 0; i < n && ok; ++i) {
        const mr_graph* g = gs[i];
        ok = g->rs_is_sr && g->traces_nonempty && !g->force_tile && g->cov_ready && g->N > 0 && g->T > 0 &&
             g->N <= FX_NMAX && g->N + 1 <= TP_LSCAN && g->nnz_rs == g->nnz_sr && g->nnz_sr < (1ll << 31) &&
             tr_su_fits(g->N) &&
             (int64_t)g->T < (int64_t)num_cus() * TRB * TR_PER_SMALL * 4;
    }
    if (!ok) {
        for (int i = 0; i < n; ++i) MR_TRY(mr_graph_prepare(ctx, gs[i]));
        return MR_OK;
    }
    for (int i = 0; i < n; ++i) {   // (the batched layout keeps every op in the id chunks)
        gs[i]->nhr = 0;
        gs[i]->hmask.reset();
    }
    hipStream_t st = ctx->stream;
    keep.assign((size_t)n * sizeof(PDev), 0);
    PDev* hp = reinterpret_cast<PDev*>(keep.data());
    std::vector<DBuf<int32_t>> trz((size_t)n);
    std::vector<DBuf<int64_t>> c64((size_t)n);
    int32_t bgc = 0, bth = 0, bcs = 0, bfl = 0, nbin_max = 0;
    int64_t st_words = 0;
    for (int i = 0; i < n; ++i) {
        mr_graph* g = gs[i];
        const int32_t N = g->N, T = g->T, W = cdiv(T, WAVE);
        const int64_t nnz = g->nnz_sr;
        MR_TRY(g->w_t.alloc(ctx, (size_t)T));
        MR_TRY(g->u_o.alloc(ctx, (size_t)N));
        MR_TRY(g->pw.alloc(ctx, (size_t)N));
        MR_TRY(g->rs16.alloc(ctx, (size_t)nnz + 8));
        const int32_t nz = 2 * (N + 1);
        MR_TRY(trz[(size_t)i].alloc(ctx, (size_t)nz));
        MR_TRY(c64[(size_t)i].alloc(ctx, (size_t)W + 1));
        MR_TRY(g->tperm.alloc(ctx, (size_t)std::max(T, 1)));
        MR_TRY(g->tpos.alloc(ctx, (size_t)std::max(T, 1)));
        g->tpos_ok = true;   // (k_tr_place_b writes the inverse beside tperm)
        MR_TRY(g->w_tp.alloc(ctx, (size_t)std::max(T, 1)));
        MR_TRY(g->coff.alloc(ctx, (size_t)W + 1));
        const int64_t nch = 2 * (int64_t)W + (nnz / WAVE + 2 * (int64_t)N) / 4 + 2;   // as tr_layout
        MR_TRY(g->tids.alloc(ctx, (size_t)std::max<int64_t>(nch, 1) * WAVE * 4));
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
        PDev& v = hp[i];
        v.T = T;
        v.N = N;
        v.nbin = N + 1;
        v.W = W;
        v.nz = nz;
        v.nnz = nnz;
        v.n_cs = (int32_t)std::max<int64_t>(cdiv((int64_t)W, TS_TILE), 1);
        v.st_off = st_words;
        st_words += v.n_cs;
        v.len_t = g->len_t.p;
        v.len_o = g->len_o.p;
        v.nchild = g->nchild.p;
        v.rs_ops = g->rs_ops.p;
        v.rs_off = g->rs_off.p;
        v.w_t = g->w_t.p;
        v.u_o = g->u_o.p;
        v.pw = g->pw.p;
        v.w_tp = g->w_tp.p;
        v.rs16 = g->rs16.p;
        v.tids = g->tids.p;
        v.trz = trz[(size_t)i].p;
        v.tperm = g->tperm.p;
        v.tpos = g->tpos.p;
        v.coff = g->coff.p;
        v.c64 = c64[(size_t)i].p;
        v.b_gc = bgc;
        bgc += cdiv(std::max<int64_t>({(int64_t)T, (int64_t)N, cdiv(nnz, 4), (int64_t)nz}), 256);
        v.b_th = bth;
        bth += cdiv(T, (int64_t)TRB * TR_PER_SMALL);
        v.b_cs = bcs;
        bcs += v.n_cs;
        v.b_fill = bfl;
        bfl += cdiv((int64_t)W * WAVE, 256);
        nbin_max = std::max(nbin_max, N + 1);
    }
    DBuf<PDev> dpd;
    MR_TRY(dpd.upload(ctx, hp, (size_t)n));
    unsigned long long* dst = nullptr;
    uint64_t epoch = 0;
    MR_TRY(mr_dl_status(ctx, st_words, &dst, &epoch));
    hipLaunchKernelGGL(k_graph_consts_b, dim3(bgc), dim3(256), 0, st, dpd.p, n);
    hipLaunchKernelGGL(k_tr_hist_b, dim3(bth), dim3(TRB), (size_t)nbin_max * sizeof(int32_t), st, dpd.p, n);
    hipLaunchKernelGGL(k_tr_place_b, dim3(bth), dim3(TRB), 2 * (size_t)nbin_max * sizeof(int32_t), st, dpd.p, n);
    hipLaunchKernelGGL(k_tr_chunk_scan_b, dim3(bcs), dim3(TS_T), 0, st, dpd.p, n, dst, epoch);
    hipLaunchKernelGGL(k_tr_fill_b, dim3(bfl), dim3(256), 0, st, dpd.p, n);
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;   // (scratch returns to the stream-ordered pool)
}

int mr_graph_prepare(mr_ctx* ctx, mr_graph* g) {
    hipStream_t st = ctx->stream;
    const int32_t N = g->N, T = g->T;
    const int64_t nnz = g->nnz_sr;
    if (nnz >= (1ll << 31)) return mr_fail(ctx, MR_ERR_ARG, "more than 2^31 (trace, op) pairs on one device: shard the traces");
    MR_TRY(g->w_t.alloc(ctx, (size_t)T));
    MR_TRY(g->u_o.alloc(ctx, (size_t)N));
    MR_TRY(g->pw.alloc(ctx, (size_t)N));
    if (!g->cov_ready) MR_TRY(g->cov.alloc(ctx, (size_t)N));
    const bool u16 = N <= 65536 && g->nnz_rs;
    if (u16) MR_TRY(g->rs16.alloc(ctx, (size_t)g->nnz_rs + 8));
    // the fused layout's histogram and slot counters, cleared by the same launch
    DBuf<int32_t> trz;
    const int32_t nz = N <= FX_NMAX ? 2 * (N + 1) : 0;
    if (nz) MR_TRY(trz.alloc(ctx, (size_t)nz));
    const int64_t nc = std::max<int64_t>({(int64_t)T, (int64_t)N, u16 ? cdiv(g->nnz_rs, 4) : 0, (int64_t)nz});
    if (nc)
        hipLaunchKernelGGL(k_graph_consts, dim3(cdiv(nc, 256)), dim3(256), 0, st, g->len_t.p, g->w_t.p, T, g->len_o.p,
                           g->nchild.p, g->u_o.p, g->pw.p, N, g->rs_ops.p, u16 ? g->nnz_rs : 0,
                           u16 ? g->rs16.p : (uint16_t*)nullptr, trz.p, nz);
    g->relabeled = false;   // (set below for fused graphs that need it)
    g->wide = false;
    g->NA = N;
    static const bool no_fused = getenv("MR_NO_FUSED") != nullptr;   // A/B knob: force the tile path
    static const bool no_wide = getenv("MR_NO_WIDE") != nullptr;     // A/B knob: N > FX_NMAX on the tile path
    const bool fusable = !no_fused && !g->force_tile && g->rs_is_sr && g->traces_nonempty;
    if (fusable && !no_wide && N > FX_NMAX && (int64_t)N <= (int64_t)WIDE_NA + (int64_t)WIDE_RMAX * WIDE_RW_MAX) {
        g->fused = true;
        return wide_prepare(ctx, g);
    }
    g->fused = fusable && N <= FX_NMAX;
    if (g->fused) {   // no P_sr tiles: the fused iteration reads the trace-major ids only
        if (!g->cov_ready) MR_TRY_HIP(ctx, hipMemsetAsync(g->cov.p, 0, (size_t)std::max(N, 1) * sizeof(int32_t), st));
        if (nnz && N && !g->cov_ready)
            hipLaunchKernelGGL(k_cov_hist, dim3(cdiv(nnz, 256 * 64)), dim3(256), (size_t)N * sizeof(int32_t), st,
                               g->rs16.p, nnz, N, g->cov.p);
        // su does not fit in LDS beside the accumulators: relabel ops by descending coverage so
        // k_tr_a stages the su of the most covered ops (ops [0, n_hot)) and gathers the rest.
        // The kinds keep rs16 (original labels, the same hash on every rank); only the
        // iteration's id stream (rsp), su and the partial rows use the new labels.
        g->relabeled = !tr_su_fits(N);
        if (g->relabeled) {
            DBuf<uint64_t> key;
            DBuf<int32_t> inv;
            MR_TRY(key.alloc(ctx, (size_t)N));
            MR_TRY(inv.alloc(ctx, (size_t)N));
            MR_TRY(g->perm.alloc(ctx, (size_t)N));
            MR_TRY(g->rsp.alloc(ctx, (size_t)nnz + 8));
            hipLaunchKernelGGL(k_relabel_keys, dim3(cdiv(N, 256)), dim3(256), 0, st, g->cov.p, N, key.p);
            SortScratch ws;
            MR_TRY(mr_radix_sort(ctx, key.p, nullptr, N, 46, ws));
            hipLaunchKernelGGL(k_relabel_perm, dim3(cdiv(N, 256)), dim3(256), 0, st, key.p, N, g->perm.p, inv.p);
            if (nnz) hipLaunchKernelGGL(k_relabel_ids, dim3(cdiv(nnz, 256)), dim3(256), 0, st, g->rs16.p, nnz, inv.p, g->rsp.p);
        } else {
            g->perm.reset();
            g->rsp.reset();
        }
        MR_TRY(tr_layout(ctx, g, g->rs_off.p, g->relabeled ? g->rsp.p : g->rs16.p, N, nnz, trz.p));
        g->n_tiles = 0;
        g->n_pairs = 0;
        MR_TRY_HIP(ctx, hipGetLastError());
        return MR_OK;
    }
    // tiles: ~256 of them when T allows, 256..4096 traces each
    int ts = TSHIFT_MIN;
    while (ts < TSHIFT_MAX && ((int64_t)T >> ts) > 256) ++ts;
    g->tshift = ts;
    g->n_tiles = T ? cdiv(T, (int64_t)1 << ts) : 0;
    const int32_t NTL = g->n_tiles;
    const int nb = std::max(1, bits_for((uint64_t)std::max(N - 1, 0)));
    const int64_t* off = g->rs_is_sr ? g->rs_off.p : g->srt_off.p;
    const int32_t* ops = g->rs_is_sr ? g->rs_ops.p : g->srt_ops.p;
    MR_TRY(g->tl_ltr.alloc(ctx, (size_t)nnz));
    MR_TRY(g->tile_pr0.alloc(ctx, (size_t)NTL + 1));
    MR_TRY(g->tile_lp0.alloc(ctx, (size_t)NTL + 1));
    MR_TRY(g->op_pr_off.alloc(ctx, (size_t)N + 1));
    int64_t np = 0;
    DBuf<int32_t> pr_tile;
    {
        DBuf<uint64_t> key;
        DBuf<uint32_t> val;
        DBuf<int32_t> head;
        DBuf<int64_t> hpos, tmp;
        MR_TRY(key.alloc(ctx, (size_t)nnz));
        MR_TRY(val.alloc(ctx, (size_t)nnz));
        MR_TRY(head.alloc(ctx, (size_t)nnz));
        MR_TRY(hpos.alloc(ctx, (size_t)nnz + 1));
        MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(std::max<int64_t>(nnz, 1))));
        if (T) hipLaunchKernelGGL(k_tile_keys, dim3(cdiv(T, 256)), dim3(256), 0, st, off, ops, T, ts, nb, key.p, val.p);
        SortScratch ws;
        MR_TRY(mr_radix_sort(ctx, key.p, val.p, nnz, nb + bits_for((uint64_t)std::max(NTL - 1, 0)), ws));
        if (nnz) hipLaunchKernelGGL(k_key_heads, dim3(cdiv(nnz, 256)), dim3(256), 0, st, key.p, nnz, head.p);
        MR_TRY(mr_exclusive_scan_i32(ctx, head.p, hpos.p, nnz, tmp.p));
        MR_TRY_HIP(ctx, hipMemcpyAsync(&np, hpos.p + nnz, sizeof np, hipMemcpyDeviceToHost, st));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
        g->n_pairs = np;
        MR_TRY(g->pr_op.alloc(ctx, (size_t)np));
        MR_TRY(g->pr_beg.alloc(ctx, (size_t)np + 1));
        MR_TRY(pr_tile.alloc(ctx, (size_t)np));
        if (nnz)
            hipLaunchKernelGGL(k_tile_pairs, dim3(cdiv(nnz, 256)), dim3(256), 0, st, key.p, val.p, head.p, hpos.p, nnz, nb,
                               g->tl_ltr.p, g->pr_op.p, g->pr_beg.p, pr_tile.p);
        else
            MR_TRY_HIP(ctx, hipMemsetAsync(g->pr_beg.p, 0, sizeof(int64_t), st));
    }
    hipLaunchKernelGGL(k_lower_bound<int32_t>, dim3(cdiv(NTL + 1, 256)), dim3(256), 0, st, pr_tile.p, np,
                       (const int64_t*)nullptr, NTL, g->tile_pr0.p);
    // long pairs (> LONG_PAIR entries) get a whole wave; listed per tile
    MR_TRY(g->lp.alloc(ctx, (size_t)std::max<int64_t>(np, 1)));
    {
        DBuf<int32_t> lflag, lp_tile;
        DBuf<int64_t> lpos, tmp;
        MR_TRY(lflag.alloc(ctx, (size_t)np));
        MR_TRY(lpos.alloc(ctx, (size_t)np + 1));
        MR_TRY(lp_tile.alloc(ctx, (size_t)std::max<int64_t>(np, 1)));
        MR_TRY(tmp.alloc(ctx, (size_t)scan_tmp_elems(std::max<int64_t>(np, 1))));
        if (np) hipLaunchKernelGGL(k_long_flags, dim3(cdiv(np, 256)), dim3(256), 0, st, g->pr_beg.p, np, lflag.p);
        MR_TRY(mr_exclusive_scan_i32(ctx, lflag.p, lpos.p, np, tmp.p));
        if (np)
            hipLaunchKernelGGL(k_long_list, dim3(cdiv(np, 256)), dim3(256), 0, st, lflag.p, lpos.p, pr_tile.p, np, g->lp.p,
                               lp_tile.p);
        hipLaunchKernelGGL(k_lower_bound<int32_t>, dim3(cdiv(NTL + 1, 256)), dim3(256), 0, st, lp_tile.p, (int64_t)0,
                           lpos.p + np, NTL, g->tile_lp0.p);
    }
    // op-major order of the pairs (tile order within an op): the s' reduction order
    MR_TRY(g->op_pr.alloc(ctx, (size_t)np));
    {
        DBuf<uint64_t> key;
        DBuf<uint32_t> val;
        DBuf<int32_t> okey;
        MR_TRY(key.alloc(ctx, (size_t)np));
        MR_TRY(val.alloc(ctx, (size_t)np));
        MR_TRY(okey.alloc(ctx, (size_t)np));
        if (np) hipLaunchKernelGGL(k_pair_op_keys, dim3(cdiv(np, 256)), dim3(256), 0, st, g->pr_op.p, np, key.p, val.p);
        SortScratch ws;
        MR_TRY(mr_radix_sort(ctx, key.p, val.p, np, nb, ws));
        if (np) hipLaunchKernelGGL(k_op_pairs, dim3(cdiv(np, 256)), dim3(256), 0, st, key.p, val.p, np, g->op_pr.p, okey.p);
        hipLaunchKernelGGL(k_lower_bound<int32_t>, dim3(cdiv(N + 1, 256)), dim3(256), 0, st, okey.p, np,
                           (const int64_t*)nullptr, N, g->op_pr_off.p);
    }
    if (N) hipLaunchKernelGGL(k_cov, dim3(cdiv(N, 256)), dim3(256), 0, st, g->op_pr_off.p, g->op_pr.p, g->pr_beg.p, N, g->cov.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;   // scratch returns to the stream-ordered pool: no sync needed
}
