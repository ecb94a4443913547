// The layout-order window batch: the first tier of the window build (win_chunk_build_async,
// mr_detect.hip) for tables with a layout order (mr_spans.lo_ok, mr_lo_fits) unless MR_NO_LO_WIN
// is set -- the detector (anormaly_detector.py:44-84) and both graphs of each window
// (get_pagerank_graph, preprocess_data.py:146-171) from the table's layout-ordered copies, ending
// in the join-pair and node-order launches it shares with the two-graph batch (mr_build_win.hip).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "mr_build_internal.h"

// A window's graphs tile their traces in the table's layout order (mr_spans.lo_*: by distinct
// pod-op count, then code -- window-independent, built with the index).  The selection runs over
// that order: each selected trace's position in its graph is its rank among the graph's traces
// there (look-back scan), pinv[position] = its layout index, and its kind class is counted
// (pagerank.py:54-66's class size = the histogram of the graph's class ids).  No trace-major
// incidence, no per-graph sort by length, no kind hashing: the prepare reads each position's
// codes from the layout-ordered u16 lists (near-contiguous for a tile) and relabels them.
constexpr int LB_T = 512;                  // k_lo_build_b threads (a block: a layout range of mr_spans.lo_bstart)
constexpr int64_t LB_LDS_WORDS = 30720;   // its two graphs' histograms and the service-op thresholds (120 KB)
constexpr int32_t LB_A3MAX = 4096;        // service-op thresholds in LDS (8 B each)
// (the two-graph batch's limits hold a fortiori: a table that fits here falls back to it)
static_assert(LB_LDS_WORDS <= IX_LDS_WORDS, "mr_lo_fits: within mr_ix2_fits");
bool mr_lo_fits(const mr_spans* sp) {
    return sp->indexed && mr_ix2_fits(sp) && sp->n_edge_keys <= NS_EMAX &&
           2 * (3 * (int64_t)sp->n_podops + sp->n_edge_keys) + 2 * (int64_t)sp->n_svcops <= LB_LDS_WORDS &&
           sp->n_svcops <= LB_A3MAX && sp->n_traces <= (1 << 24);
}
// Per window, in its table's layout order: the detector (anormaly_detector.py:44-84 as
// detect_block: a trace's expect summed sequentially over its service-ops in name order, T14),
// the selection of both graphs (T1 swap: state 2 -> graph 0, 1 -> graph 1: a side byte per layout
// index, k_lo_pos_b's input) and each class's count, and both graphs' per-pod-op span counts /
// first rows / coverage and per-edge-id multiplicities (get_pagerank_graph's len_o, node order
// and children multisets, preprocess_data.py:146-171) in LDS, written once per block as a partial
// row (the first row as INT_MAX - row, combined by max) that k_lo_reduce_b combines per window.
// A block is a layout range of at most LO_BT_MAX traces and LO_BE entries (mr_spans.lo_bstart):
// a thread per trace for the detector, then every wave of the block over the range's entries (a
// lane per entry, coalesced, four rounds of loads in flight), each entry's trace found from the
// traces' starts in LDS.  No block waits for another.
struct IxWinLoB {
    const int32_t *lo_tr, *lo_len, *lo_kid, *lo_first, *bstart;
    const int64_t *lo_off, *lsv_off, *le_off;
    const uint16_t *lo16, *lo_cnt;
    const uint32_t *lsv, *le;
    const long long *lo_ts, *lo_te, *lo_mx;
    const double* a3;
    const uint8_t* a3v;
    int64_t t0, t1;
    uint8_t* state;                  // by trace code (k_ix_cross2_b reads it)
    int8_t* side;                    // by layout index: 0 / 1 graph, -1 none
    unsigned long long* counts;      // detector counter shards (3 * CSH, zeroed)
    int32_t NT, NP, nek, nsvc;
    uint32_t* kcnt[2];               // kind class histograms (zeroed)
    int64_t* tot[2];                 // [T, nnz] (zeroed)
    uint32_t* rows;                  // partial rows [block][graph][cnt NP | cov NP | INT_MAX - first NP | edges nek]
    int32_t cmp, pad_;               // complement form: graph 1's histogram holds the traces in NEITHER graph
    uint32_t* nrow;                  // ... added into this zeroed row by the blocks that have any (no partial row)
};
// the build's first LDS region: both graphs' histograms, and before them (aliased) the detector's
// products of a round -- at least 2048 of them
__host__ __device__ __forceinline__ size_t lo_region0(size_t gbytes) {
    return 2 * gbytes > (size_t)2048 * 8 ? 2 * gbytes : (size_t)2048 * 8;
}
constexpr int LB_R = 4;   // entry rounds per batch (their loads in flight together)
// the block-relative trace whose entries [st[t], st[t+1]) hold entry e (st ascending, st[0] = 0,
// st[nt] = the range's entries): a division when the range's traces all have n entries (the layout
// sorts by entry count: the usual case), else a binary search in LDS
__device__ __forceinline__ int32_t lo_trace_of(uint32_t e, uint32_t n, const uint32_t* st, int32_t nt) {
    if (n > 0) return (int32_t)(e / n);
    // a fixed number of steps (LO_BT_MAX = 1024 traces): the searches of a batch's rounds are
    // independent chains the compiler can interleave (a data-dependent loop would run them one by one)
    int32_t lo = 0;
#pragma unroll
    for (int32_t step = LO_BT_MAX / 2; step >= 1; step >>= 1) {
        const int32_t mid = lo + step;
        lo = mid < nt && st[mid] <= e ? mid : lo;
    }
    return lo;
}
__global__ void __launch_bounds__(LB_T, 6) k_lo_build_b(IxBatch<IxWinLoB> a) {
    // per graph g: [cnt | cov << 32] u64 x NP, then INT_MAX - first row x NP, then edge counts x
    // nek; then the service-op thresholds (0 where a3v is false: adding +0.0 leaves expect as is)
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    __shared__ uint32_t pst[LO_BT_MAX + 1], est[LO_BT_MAX + 1];   // the traces' first entries (relative)
    __shared__ int8_t ss[LO_BT_MAX];
    __shared__ unsigned long long bc[5][LB_T / WAVE];
    __shared__ uint16_t kl[LO_BT_MAX];   // complement form: the range's traces outside graph 1
    __shared__ uint32_t nkl, nnei;
    const int k = ixb_pick(a.b0, a.n);
    const IxWinLoB& w = a.w[k];
    const int32_t blk = (int32_t)blockIdx.x - a.b0[k];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const int32_t NP = w.NP, nek = w.nek;
    const size_t gbytes = ((size_t)NP * 12 + (size_t)nek * 4 + 15) / 16 * 16;   // one graph's histograms
    const size_t reg0 = lo_region0(gbytes);   // the histograms; before them, the detector's products
    double* la3 = (double*)(lraw + reg0);
    double* prod = (double*)lraw;
    const uint32_t cap = (uint32_t)(reg0 / 8 / LB_T * LB_T);   // products per round
    for (int32_t c = tid; c < w.nsvc; c += LB_T) la3[c] = w.a3v[c] ? w.a3[c] : 0.0;
    const int32_t T0 = w.bstart[blk], nt = w.bstart[blk + 1] - T0;
    const int64_t P0 = w.lo_off[T0], Q0 = w.le_off[T0], V0 = w.lsv_off[T0];
    const uint32_t np = (uint32_t)(w.lo_off[T0 + nt] - P0), nq = (uint32_t)(w.le_off[T0 + nt] - Q0);
    const uint32_t nv = (uint32_t)(w.lsv_off[T0 + nt] - V0);
    if (tid == 0) {
        pst[nt] = np;
        est[nt] = nq;
        nkl = nnei = 0u;
    }
    // this thread's traces: slot s holds trace s * LB_T + tid of the range (64 consecutive per wave)
    constexpr int NS = LO_BT_MAX / LB_T;
    uint32_t va[NS], vb[NS];
    bool act[NS];
    double expect[NS];
    long long mx[NS];
    unsigned long long rows = 0;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int32_t t = q * LB_T + tid;
        const bool valid = t < nt;
        const int64_t i = (int64_t)T0 + (valid ? t : nt - 1);   // (clamped)
        const int32_t len = w.lo_len[i];
        const long long ts = w.lo_ts[i], te = w.lo_te[i];
        mx[q] = w.lo_mx[i];
        va[q] = (uint32_t)(w.lsv_off[i] - V0);
        vb[q] = (uint32_t)(w.lsv_off[i + 1] - V0);
        const bool in = valid && len > 0 && ts >= w.t0 && te <= w.t1;
        rows += in ? (unsigned long long)len : 0ull;
        act[q] = in && mx[q] > 0;   // grouped[grouped['duration'] > 0] (preprocess_data.py:117)
        expect[q] = 0.0;
    }
    __syncthreads();   // (the thresholds in LDS)
    // the detector's expect (anormaly_detector.py:63-67), sequential in name order per trace (T14):
    // the range's service-op products staged in LDS a round at a time (coalesced loads, every load of
    // a round in flight), each lane then adding its own trace's products of the round in order --
    // the same products, the same sequential sums as a lane walking its trace alone
    for (uint32_t r0 = 0; r0 < nv; r0 += cap) {
        const uint32_t rn = min(cap, nv - r0);
        constexpr int LU = 8;
        for (uint32_t x0 = 0; x0 < rn; x0 += LU * LB_T) {
            uint32_t v[LU];
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const uint32_t x = x0 + (uint32_t)(u * LB_T + tid);
                v[u] = w.lsv[V0 + (int64_t)(r0 + min(x, rn - 1))];
            }
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const uint32_t x = x0 + (uint32_t)(u * LB_T + tid);
                if (x < rn) prod[x] = (double)(v[u] >> 16) * la3[v[u] & 0xffffu];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NS; ++q)
            if (act[q]) {
                const uint32_t lo = max(va[q], r0), hi = min(vb[q], r0 + rn);
                for (uint32_t j = lo; j < hi; j += 8) {   // eight LDS reads in flight, then the adds in order
                    double p8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) p8[u] = prod[min(j + u, hi - 1) - r0];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (j + u < hi) expect[q] += p8[u];
                }
            }
        __syncthreads();
    }
    for (size_t x = (size_t)tid * 4; x < reg0; x += (size_t)LB_T * 4) *(uint32_t*)(lraw + x) = 0u;
    unsigned long long nab = 0, nno = 0, nz0 = 0, nz1 = 0;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int32_t t = q * LB_T + tid;
        const bool valid = t < nt;
        const int64_t i = (int64_t)T0 + (valid ? t : nt - 1);   // (clamped)
        const int32_t kid0 = w.lo_kid[i], tr = w.lo_tr[i];
        const int64_t pa = w.lo_off[i], pb = w.lo_off[i + 1], ea = w.le_off[i];
        const int stt = act[q] ? ((double)mx[q] / 1000.0 > expect[q] ? 2 : 1) : 0;   // :58, :69
        const int s_ = valid ? (stt == 2 ? 0 : stt == 1 ? 1 : -1) : -1;
        if (valid) {
            w.state[tr] = (uint8_t)stt;
            w.side[i] = (int8_t)s_;
            ss[t] = (int8_t)s_;
            pst[t] = (uint32_t)(pa - P0);
            est[t] = (uint32_t)(ea - Q0);
        }
        nab += stt == 2;
        nno += stt == 1;
        if (s_ == 0) nz0 += (unsigned long long)(pb - pa);
        else if (s_ == 1) nz1 += (unsigned long long)(pb - pa);
        // kind classes are runs of the layout: one add per (run, graph) of the wave
        const int kid = valid ? kid0 : -1;
        const int kp = __shfl_up(kid, 1, WAVE);
        const bool hd = kid >= 0 && (lane == 0 || kp != kid);
        const unsigned long long H = __ballot(hd), B0 = __ballot(s_ == 0), B1 = __ballot(s_ == 1);
        if (hd) {
            const unsigned long long above = lane == WAVE - 1 ? 0ull : H & (~0ull << (lane + 1));
            const unsigned long long run = (above ? (above & (0ull - above)) - 1ull : ~0ull) & (~0ull << lane);
            const uint32_t c0 = (uint32_t)__popcll(B0 & run), c1 = (uint32_t)__popcll(B1 & run);
            if (c0) atomicAdd(&w.kcnt[0][kid], c0);
            if (c1) atomicAdd(&w.kcnt[1][kid], c1);
        }
        if (w.cmp) {   // the traces whose entries this form walks: one list slot each, a wave's together
            const bool keep = valid && s_ != 1;
            const unsigned long long K = __ballot(keep);
            uint32_t base = 0u;
            if (lane == 0 && K) base = atomicAdd(&nkl, (uint32_t)__popcll(K));
            if (lane == 0 && (K & ~B0)) atomicAdd(&nnei, (uint32_t)__popcll(K & ~B0));
            base = (uint32_t)__shfl((int)base, 0, WAVE);
            if (keep) kl[base + (uint32_t)__popcll(K & ((1ull << lane) - 1ull))] = (uint16_t)t;
        }
    }
    __syncthreads();
    // the range's pod-op and join entries, each to its trace's graph.  A range of short traces (the
    // longest -- the layout sorts by count, so the last -- of <= LB_LANE pod-ops): a lane per trace
    // walks its own entries, all loads out at once, no lookups, each trace's entries rotated by its
    // index (a run of identical traces would otherwise add into the same word in the same round).
    // Else every wave over the range's entries, a lane per entry, the entry's trace looked up.
    // The complement form (w.cmp) walks the entries of the listed traces only -- graph 0's into
    // histogram 0, those of the traces in neither graph into histogram 1 (no first rows: the
    // reduce subtracts both from the table's totals) -- and loads nothing of a graph-1 trace:
    // sixteen lanes per listed trace, two traces' first loads in flight per group.
    if (w.cmp) {
        constexpr int GL = 16, NG = LB_T / GL;
        const uint32_t nk = nkl, gl = (uint32_t)tid & (GL - 1);
        for (uint32_t x0 = (uint32_t)tid / GL; x0 < nk; x0 += 2 * NG) {
            uint32_t a0[2], n[2], b0e[2], m[2], pc[2], ev[2];
            int32_t fr[2];
            bool g0[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t x = x0 + (uint32_t)(u * NG);
                const int32_t t = kl[x < nk ? x : x0];
                g0[u] = ss[t] == 0;
                a0[u] = pst[t];
                n[u] = x < nk ? pst[t + 1] - a0[u] : 0u;
                b0e[u] = est[t];
                m[u] = x < nk ? est[t + 1] - b0e[u] : 0u;
                pc[u] = ev[u] = 0u;
                fr[u] = 0;
                if (gl < n[u]) {
                    const int64_t e = P0 + (int64_t)(a0[u] + gl);
                    pc[u] = (uint32_t)w.lo16[e] | ((uint32_t)w.lo_cnt[e] << 16);
                    if (g0[u]) fr[u] = w.lo_first[e];
                }
                if (gl < m[u]) ev[u] = w.le[Q0 + (int64_t)(b0e[u] + gl)];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                unsigned char* G = lraw + (g0[u] ? (size_t)0 : gbytes);
                int32_t* Gf = (int32_t*)(G + (size_t)NP * 8);
                uint32_t* Ge = (uint32_t*)(G + (size_t)NP * 12);
                for (uint32_t j = gl; j < n[u]; j += GL) {
                    if (j >= GL) {
                        const int64_t e = P0 + (int64_t)(a0[u] + j);
                        pc[u] = (uint32_t)w.lo16[e] | ((uint32_t)w.lo_cnt[e] << 16);
                        if (g0[u]) fr[u] = w.lo_first[e];
                    }
                    const uint32_t c = pc[u] & 0xffffu;
                    atomicAdd((unsigned long long*)G + c, (unsigned long long)(pc[u] >> 16) | (1ull << 32));
                    if (g0[u]) atomicMax(Gf + c, 0x7fffffff - fr[u]);
                }
                for (uint32_t j = gl; j < m[u]; j += GL) {
                    if (j >= GL) ev[u] = w.le[Q0 + (int64_t)(b0e[u] + j)];
                    atomicAdd(Ge + (ev[u] & 0xffffu), ev[u] >> 16);
                }
            }
        }
    }
    constexpr int LB_LANE = 8;
    const bool lanewise = !w.cmp && nt > 0 && pst[nt] - pst[nt - 1] <= (uint32_t)LB_LANE;
    if (lanewise) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int32_t t = q * LB_T + tid;
            const int sd = t < nt ? (int)ss[t] : -1;
            if (sd < 0) continue;
            unsigned char* G = lraw + (size_t)sd * gbytes;
            const uint32_t a0 = pst[t], n = pst[t + 1] - a0, rot = n ? (uint32_t)t % n : 0u;
            uint32_t pc[LB_LANE];
            int32_t fr[LB_LANE];
#pragma unroll
            for (int u = 0; u < LB_LANE; ++u) {
                const uint32_t j = (uint32_t)u + rot;
                const int64_t e = P0 + (int64_t)a0 + (u < (int)n ? (j >= n ? j - n : j) : 0u);
                pc[u] = (uint32_t)w.lo16[e] | ((uint32_t)w.lo_cnt[e] << 16);
                fr[u] = w.lo_first[e];
            }
#pragma unroll
            for (int u = 0; u < LB_LANE; ++u)
                if (u < (int)n) {
                    const uint32_t c = pc[u] & 0xffffu;
                    atomicAdd((unsigned long long*)G + c, (unsigned long long)(pc[u] >> 16) | (1ull << 32));
                    atomicMax((int32_t*)(G + (size_t)NP * 8) + c, 0x7fffffff - fr[u]);
                }
            const uint32_t b0e = est[t], m = est[t + 1] - b0e, rte = m ? (uint32_t)t % m : 0u;
            uint32_t* Ge = (uint32_t*)(G + (size_t)NP * 12);
            for (uint32_t u0 = 0; u0 < m; u0 += LB_LANE) {
                uint32_t ev[LB_LANE];
#pragma unroll
                for (int u = 0; u < LB_LANE; ++u) {
                    const uint32_t j = u0 + (uint32_t)u, jr = j + rte;
                    ev[u] = w.le[Q0 + (int64_t)b0e + (j < m ? (jr >= m ? jr - m : jr) : 0u)];
                }
#pragma unroll
                for (int u = 0; u < LB_LANE; ++u)
                    if (u0 + (uint32_t)u < m) atomicAdd(Ge + (ev[u] & 0xffffu), ev[u] >> 16);
            }
        }
    }
    const uint32_t n0 = nt ? pst[1 < nt ? 1 : nt] - pst[0] : 0u;
    const uint32_t npo = n0 > 0 && np == (uint32_t)nt * n0 ? n0 : 0u;   // (uniform: every trace n0 entries)
    constexpr int NW = LB_T / WAVE;
    const uint32_t nmax = lanewise || w.cmp ? 0u : max(np, nq);
    for (uint32_t b0 = (uint32_t)wv * (LB_R * WAVE); b0 < nmax; b0 += NW * LB_R * WAVE) {
        uint32_t pc[LB_R], ev[LB_R];
        int32_t fr[LB_R];
#pragma unroll
        for (int r = 0; r < LB_R; ++r) {   // (clamped: every load in bounds)
            const uint32_t o = b0 + (uint32_t)(r * WAVE + lane);
            if (b0 < np) {
                const int64_t e = P0 + (int64_t)min(o, np - 1u);
                pc[r] = (uint32_t)w.lo16[e] | ((uint32_t)w.lo_cnt[e] << 16);
                fr[r] = w.lo_first[e];
            }
            if (b0 < nq) ev[r] = w.le[Q0 + (int64_t)min(o, nq - 1u)];
        }
#pragma unroll
        for (int r = 0; r < LB_R; ++r) {
            const uint32_t o = b0 + (uint32_t)(r * WAVE + lane);
            if (o < np) {
                const int sd = ss[lo_trace_of(o, npo, pst, nt)];
                if (sd >= 0) {
                    unsigned char* G = lraw + (size_t)sd * gbytes;
                    const uint32_t c = pc[r] & 0xffffu;
                    atomicAdd((unsigned long long*)G + c, (unsigned long long)(pc[r] >> 16) | (1ull << 32));
                    atomicMax((int32_t*)(G + (size_t)NP * 8) + c, 0x7fffffff - fr[r]);
                }
            }
            if (o < nq) {
                const int sd = ss[lo_trace_of(o, 0u, est, nt)];
                if (sd >= 0)
                    atomicAdd((uint32_t*)(lraw + (size_t)sd * gbytes + (size_t)NP * 12) + (ev[r] & 0xffffu), ev[r] >> 16);
            }
        }
    }
    __syncthreads();
    {   // the detector's counts and both graphs' entry totals: per wave, per block, one add each
        unsigned long long v[5] = {nab, nno, rows, nz0, nz1};
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] += __shfl_xor(v[q], m, WAVE);
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 5; ++q) bc[q][wv] = v[q];
    }
    __syncthreads();
    if (tid < 5) {
        unsigned long long v = 0;
        for (int q = 0; q < NW; ++q) v += bc[tid][q];
        if (v) {
            if (tid < 3) atomicAdd(&w.counts[(size_t)(blk % CSH) * 3 + tid], v);
            else atomicAdd((unsigned long long*)&w.tot[tid - 3][1], v);
        }
    }
    // the block's histograms as its partial row (plain stores; k_lo_reduce_b combines the rows)
    const size_t rw = 3 * (size_t)NP + (size_t)nek;
    uint32_t* R = w.rows + (size_t)blk * 2 * rw;
    if (w.cmp && nnei != 0u) {   // (few blocks of a window that takes this form: the traces it leaves out)
        const unsigned char* G = lraw + gbytes;
        for (int32_t c = tid; c < NP; c += LB_T) {
            const unsigned long long v = ((const unsigned long long*)G)[c];
            if ((uint32_t)v) atomicAdd(&w.nrow[c], (uint32_t)v);
            if ((uint32_t)(v >> 32)) atomicAdd(&w.nrow[NP + c], (uint32_t)(v >> 32));
        }
        for (int32_t x = tid; x < nek; x += LB_T) {
            const uint32_t v = ((const uint32_t*)(G + (size_t)NP * 12))[x];
            if (v) atomicAdd(&w.nrow[3 * NP + x], v);
        }
    }
    for (int g = 0; g < (w.cmp ? 1 : 2); ++g) {
        const unsigned char* G = lraw + (size_t)g * gbytes;
        uint32_t* Rg = R + (size_t)g * rw;
        for (int32_t c = tid; c < NP; c += LB_T) {
            const unsigned long long v = ((const unsigned long long*)G)[c];
            Rg[c] = (uint32_t)v;
            Rg[NP + c] = (uint32_t)(v >> 32);
            Rg[2 * NP + c] = ((const uint32_t*)(G + (size_t)NP * 8))[c];
        }
        for (int32_t x = tid; x < nek; x += LB_T) Rg[3 * NP + x] = ((const uint32_t*)(G + (size_t)NP * 12))[x];
    }
    __syncthreads();
}
// positions: each selected trace's rank among its graph's traces in layout order (decoupled
// look-back over the side bytes), pinv[position] = layout index, staged in LDS for coalesced
// stores; the graph sizes tot[g][0]
constexpr int LP_T = 256, LP_I = 16, LP_TILE = LP_T * LP_I;
struct IxWinLoPos {
    const int8_t* side;
    int32_t NT, pad_;
    unsigned long long* st;          // look-back words: 2 chains x the window's tiles
    int32_t* pinv[2];
    int64_t* tot[2];
};
__global__ void __launch_bounds__(LP_T) k_lo_pos_b(IxBatch<IxWinLoPos> a, uint64_t epoch) {
    __shared__ int32_t sa[2][LP_T];
    __shared__ int32_t ex[2];
    __shared__ int32_t so[2][LP_TILE];
    const int k = ixb_pick(a.b0, a.n);
    const IxWinLoPos& w = a.w[k];
    const int32_t blk = (int32_t)blockIdx.x - a.b0[k], nblk = a.b0[k + 1] - a.b0[k];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int64_t base = (int64_t)blk * LP_TILE + (int64_t)tid * LP_I;
    int8_t sd[LP_I];
    if (base + LP_I <= w.NT) {   // 16 side bytes: one load
        const uint4 v = *(const uint4*)(w.side + base);
        memcpy(sd, &v, 16);
    } else {
#pragma unroll
        for (int q = 0; q < LP_I; ++q) sd[q] = base + q < w.NT ? w.side[base + q] : (int8_t)-1;
    }
    int32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int q = 0; q < LP_I; ++q) {
        c0 += sd[q] == 0;
        c1 += sd[q] == 1;
    }
    sa[0][tid] = c0;
    sa[1][tid] = c1;
    __syncthreads();
    for (int o = 1; o < LP_T; o <<= 1) {
        const int32_t v0 = tid >= o ? sa[0][tid - o] : 0, v1 = tid >= o ? sa[1][tid - o] : 0;
        __syncthreads();
        sa[0][tid] += v0;
        sa[1][tid] += v1;
        __syncthreads();
    }
    if (tid < 2 * WAVE) {   // wave g: graph g's positions
        const int g = tid / WAVE;
        const int32_t agg = sa[g][LP_T - 1];
        const int64_t e = dl_lookback_wave(w.st + (size_t)g * nblk, blk, agg, epoch);
        if (lane == 0) {
            ex[g] = (int32_t)e;
            if (blk == nblk - 1) w.tot[g][0] = e + agg;
        }
    }
    int32_t r0 = sa[0][tid] - c0, r1 = sa[1][tid] - c1;   // (block-relative)
#pragma unroll
    for (int q = 0; q < LP_I; ++q) {
        const int32_t ix = (int32_t)(base + q);
        if (sd[q] == 0) so[0][r0++] = ix;
        else if (sd[q] == 1) so[1][r1++] = ix;
    }
    __syncthreads();
    for (int g = 0; g < 2; ++g) {
        const int32_t n = sa[g][LP_T - 1], e = ex[g];
        for (int32_t x = tid; x < n; x += LP_T) w.pinv[g][e + x] = so[g][x];
    }
}
// each window's partial rows, column by column: span counts, coverage and edge multiplicities
// summed, INT_MAX - first row by max -- into the graph's words (overwritten; k_ix_cross2_b adds
// the joins across traces after)
struct IxLoRed {
    const uint32_t* rows;
    int32_t nblk, NP, nek, pad_;
    int32_t *ocnt[2], *ofinv[2], *ocov[2];
    uint32_t* gc[2];
    // complement form (tot non-null; a thread per column of BOTH graphs): graph 1's additive words
    // are the table's totals (laid out as a row) minus graph 0's column minus the word of the
    // traces in neither graph (nrow: the build's blocks added theirs).  Graph 1's first row
    // of an op it holds: the first of the op's candidates (mr_spans.lo_cand: sorted by first row,
    // a complete prefix of the op's entries) whose trace the window put into graph 1; none: *flag.
    const uint32_t* tot;
    const uint32_t* nrow;
    const int8_t* side;
    const uint64_t* ckey;
    const uint32_t* cix;
    const int64_t* coff;
    int64_t* flag;
    int32_t crb, pad2_;
};
__device__ __forceinline__ uint32_t lo_col(const uint32_t* p, size_t stride, int32_t nblk, bool mx) {
    uint32_t acc = 0;
    int32_t b = 0;
    for (; b + 8 <= nblk; b += 8) {
        uint32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = p[(size_t)(b + q) * stride];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = mx ? max(acc, v[q]) : acc + v[q];
    }
    for (; b < nblk; ++b) {
        const uint32_t v = p[(size_t)b * stride];
        acc = mx ? max(acc, v) : acc + v;
    }
    return acc;
}
__device__ __forceinline__ void lo_put(const IxLoRed& w, int g, int64_t c, uint32_t v) {
    const int32_t NP = w.NP;
    if (c < NP) w.ocnt[g][c] = (int32_t)v;
    else if (c < 2 * (int64_t)NP) w.ocov[g][c - NP] = (int32_t)v;
    else if (c < 3 * (int64_t)NP) w.ofinv[g][c - 2 * NP] = (int32_t)v;
    else w.gc[g][c - 3 * NP] = v;
}
__global__ void __launch_bounds__(256) k_lo_reduce_b(IxBatch<IxLoRed> a) {
    const int k = ixb_pick(a.b0, a.n);
    const IxLoRed& w = a.w[k];
    const int64_t rw = 3 * (int64_t)w.NP + w.nek;
    const int64_t col = (int64_t)((int32_t)blockIdx.x - a.b0[k]) * 256 + threadIdx.x;
    const size_t stride = 2 * (size_t)rw;
    if (w.tot == nullptr) {   // direct form: a thread per (graph, column)
        if (col >= 2 * rw) return;
        const int g = (int)(col / rw);
        const int64_t c = col - (int64_t)g * rw;
        const bool mx = c >= 2 * (int64_t)w.NP && c < 3 * (int64_t)w.NP;
        lo_put(w, g, c, lo_col(w.rows + col, stride, w.nblk, mx));
        return;
    }
    if (col >= rw) return;
    const bool mx = col >= 2 * (int64_t)w.NP && col < 3 * (int64_t)w.NP;
    const uint32_t a0 = lo_col(w.rows + col, stride, w.nblk, mx);
    lo_put(w, 0, col, a0);
    if (mx) return;
    const uint32_t v1 = w.tot[col] - a0 - w.nrow[col];
    lo_put(w, 1, col, v1);
    if (col < w.NP && v1 > 0u) {
        // (one thread, a chain of dependent reads: at most LO_CMP_SCAN candidates -- where 93 % of the
        // traces are normal the first or second is one; past the cap the window is rebuilt like one whose
        // candidates ran out)
        int32_t fi = 0;
        const int64_t j1 = min(w.coff[col + 1], w.coff[col] + (int64_t)LO_CMP_SCAN);
        for (int64_t j = w.coff[col]; j < j1; ++j)
            if (w.side[w.cix[j]] == 1) {
                fi = 0x7fffffff - (int32_t)(uint32_t)(w.ckey[j] & ((1ull << w.crb) - 1ull));
                break;
            }
        w.ofinv[1][col] = fi;
        if (fi == 0) *w.flag = 1;
    }
}

// Per window (n <= IXW): k_lo_build_b, the rare joins across traces, the node order / P_ss / op
// constants (k_nodes_small2_b): sizes of graph j of window k to d_outs[k] + 8 j (N, E, overflow,
// T, nnz; words 5 / 6: the build's totals).  zw[k]: the window's zeroed words, lo_zero_words(sp)
// of them.  MR_ERR_STATE: a window outside the limits (the caller takes mr_ix_launch2_batch).
int64_t mr_lo_zero_words(const mr_spans* sp) {
    // per graph the kind histogram and the graph's words; then the complement form's row of the traces in
    // neither graph (a partial row's layout)
    return 2 * ((int64_t)std::max(sp->lo_nk, 1) + 3 * (int64_t)sp->n_podops + std::max<int64_t>(sp->n_edge_keys, 1)) +
           3 * (int64_t)sp->n_podops + std::max<int64_t>(sp->n_edge_keys, 1);
}
// an upper bound of the table's traces that the window [t0, t1] leaves out of both graphs, from the
// time summary: the traces no window selects, every start bucket that reaches below t0 and every
// end bucket that reaches above t1
static int64_t lo_cmp_out_bound(const mr_spans* sp, int64_t t0, int64_t t1) {
    int64_t out = sp->lo_ninact;
    for (int b = 0; b < 64; ++b) {
        const __int128 lo = (__int128)sp->lo_tmin + (__int128)b * sp->lo_tbw;
        const __int128 hi = std::min<__int128>(lo + sp->lo_tbw - 1, sp->lo_tmax);   // (no end lies past lo_tmax)
        if (lo < (__int128)t0) out += sp->lo_hts[b];
        if (hi > (__int128)t1) out += sp->lo_hte[b];
    }
    return out;
}
static std::atomic<int64_t> g_lo_cmp_windows{0}, g_lo_cmp_rebuilt{0};
void mr_lo_cmp_counts(int64_t* n_cmp, int64_t* n_rebuilt) {
    if (n_cmp) *n_cmp = g_lo_cmp_windows.load();
    if (n_rebuilt) *n_rebuilt = g_lo_cmp_rebuilt.load();
}
void mr_lo_cmp_note_rebuild() { ++g_lo_cmp_rebuilt; }
extern "C" int mr_lo_complement_counts(int64_t* n_complement, int64_t* n_rebuilt) {
    mr_lo_cmp_counts(n_complement, n_rebuilt);
    return MR_OK;
}
int mr_lo_launch_batch(mr_ctx* ctx, int n, const mr_spans* const* sps, mr_graph* const* g0s, mr_graph* const* g1s,
                       IxBuild* const* b0s, IxBuild* const* b1s, int64_t* const* d_outs, const DetIn* dets,
                       uint32_t* const* zw, bool force_direct) {
    if (n < 1 || n > IXW || getenv("MR_NO_IX2") != nullptr) return MR_ERR_STATE;
    for (int k = 0; k < n; ++k)
        if (!sps[k]->lo_ok || !mr_lo_fits(sps[k])) return MR_ERR_STATE;
    hipStream_t st = ctx->stream;
    const char* ce = getenv("MR_LO_COMPLEMENT");   // (read per call: 0 direct, 1 complement, else by the summary)
    const int cmode = force_direct || (ce && ce[0] == '0') ? 0 : ce && ce[0] == '1' ? 1 : -1;
    std::vector<char> cmps((size_t)n);
    IxBatch<IxWinLoB> ab{};
    IxBatch<IxLoRed> ar{};
    IxBatch<IxWinLoPos> ap{};
    IxBatch<IxWinCross> ac{};
    IxBatch<IxWinNodes> an{};
    ab.n = ar.n = ap.n = ac.n = an.n = n;
    int32_t bb = 0, bc = 0, br = 0, bp = 0;
    int64_t rwords = 0, sbytes = 0;
    std::vector<int64_t> roff((size_t)n), soff((size_t)n);
    size_t lds = 4;
    int64_t words = 0;
    std::vector<int64_t> woff((size_t)n);
    for (int k = 0; k < n; ++k) {
        const mr_spans* sp = sps[k];
        const int32_t NT = sp->n_traces, NP = sp->n_podops;
        const int64_t nek = sp->n_edge_keys, nk = std::max(sp->lo_nk, 1);
        IxSide2 xs;
        NsArgs2 na;
        IxBuild* b[2] = {b0s[k], b1s[k]};
        mr_graph* g[2] = {g0s[k], g1s[k]};
        IxWinLoB& L = ab.w[k];
        const int64_t per = nk + 3 * (int64_t)NP + std::max<int64_t>(nek, 1);   // zeroed words per graph
        for (int j = 0; j < 2; ++j) {
            IxBuild& B = *b[j];
            mr_graph* G = g[j];
            B.dense = true;
            B.small = true;
            B.ecap = (uint64_t)nek;
            B.gkp = sp->ekey.p;
            uint32_t* z = zw[k] + j * per;
            B.kcnt = z;
            int32_t* ocnt = (int32_t*)(z + nk);
            int32_t* ofinv = ocnt + NP;
            int32_t* ocov = ofinv + NP;
            uint32_t* gc = (uint32_t*)(ocov + NP);
            MR_TRY(B.pinv.alloc(ctx, std::max(NT, 1)));
            MR_TRY(mr_ix_graph_buffers(ctx, NP, B, G));
            MR_TRY(G->u_o.alloc(ctx, std::max(NP, 1)));
            MR_TRY(G->pw.alloc(ctx, std::max(NP, 1)));
            xs.g[j] = IxSide{nullptr, ocnt, ofinv, ocov, nullptr, nullptr, gc};
            int64_t* out = d_outs[k] + 8 * j;
            na.g[j] = NsArgs{gc, ocnt, ofinv, ocov, B.node_of_code.p, G->node_podop.p, G->len_o.p, G->nchild.p, G->cov.p,
                             G->ss_par.p, G->ss_off.p, out + 5, out + 6, nullptr, out, G->u_o.p, G->pw.p, 1};
            ap.w[k].pinv[j] = B.pinv.p;
            ap.w[k].tot[j] = out + 5;
            L.kcnt[j] = B.kcnt;
            L.tot[j] = out + 5;
            IxLoRed& R = ar.w[k];
            R.ocnt[j] = ocnt;
            R.ofinv[j] = ofinv;
            R.ocov[j] = ocov;
            R.gc[j] = gc;
        }
        const int32_t nt = sp->lo_nblk;
        const int64_t rw = 3 * (int64_t)NP + nek;
        roff[(size_t)k] = rwords;
        rwords += (int64_t)nt * 2 * rw;
        ar.w[k].nblk = nt;
        ar.w[k].NP = NP;
        ar.w[k].nek = (int32_t)nek;
        ar.b0[k] = br;
        const bool cmp = sp->lo_cmp_ok && cmode != 0 &&
                         (cmode == 1 || 4 * lo_cmp_out_bound(sp, dets[k].t0, dets[k].t1) <= (int64_t)NT);
        cmps[(size_t)k] = cmp;
        br += (int32_t)cdiv(cmp ? rw : 2 * rw, 256);
        const int32_t npb = (int32_t)std::max<int64_t>(cdiv((int64_t)NT, LP_TILE), 1);
        woff[(size_t)k] = words;
        words += 2 * (int64_t)npb;
        ap.b0[k] = bp;
        bp += npb;
        ap.w[k].NT = NT;
        soff[(size_t)k] = sbytes;
        sbytes += ((int64_t)NT + 15) / 16 * 16;
        ab.b0[k] = bb;
        bb += nt;
        const DetIn& d = dets[k];
        L.cmp = cmp ? 1 : 0;
        L.pad_ = 0;
        IxLoRed& R = ar.w[k];
        R.tot = cmp ? sp->lo_tot.p : nullptr;
        R.ckey = sp->lo_cand_key.p;
        R.cix = sp->lo_cand_ix.p;
        R.coff = sp->lo_cand_off.p;
        R.crb = sp->lo_cand_rb;
        R.pad2_ = 0;
        R.flag = d_outs[k] + 15;
        L.bstart = sp->lo_bstart.p;
        L.lo_tr = sp->lo_tr.p;
        L.lo_len = sp->lo_len.p;
        L.lo_kid = sp->lo_kid.p;
        L.lo_first = sp->lo_first.p;
        L.lo_off = sp->lo_off.p;
        L.lsv_off = sp->lsv_off.p;
        L.le_off = sp->le_off.p;
        L.lo16 = sp->lo16.p;
        L.lo_cnt = sp->lo_cnt.p;
        L.lsv = sp->lsv.p;
        L.le = sp->le.p;
        L.lo_ts = sp->lo_ts.p;
        L.lo_te = sp->lo_te.p;
        L.lo_mx = sp->lo_mx.p;
        L.a3 = d.a3;
        L.a3v = d.a3v;
        L.t0 = d.t0;
        L.t1 = d.t1;
        L.state = d.state;
        L.counts = d.counts;
        L.NT = NT;
        L.NP = NP;
        L.nek = (int32_t)nek;
        L.nsvc = sp->n_svcops;
        lds = std::max(lds, lo_region0(((size_t)NP * 12 + (size_t)nek * 4 + 15) / 16 * 16) + (size_t)sp->n_svcops * 8);
        ac.b0[k] = bc;
        bc += (int32_t)cdiv(sp->n_xj, 256);
        ac.w[k] = IxWinCross{d.state, sp->xj_tc.p, sp->xj_tp.p, sp->xj_eid.p, sp->n_xj, xs};
        an.b0[k] = 2 * k;
        an.w[k] = IxWinNodes{sp->ekey.p, nek, NP, 0, na};
    }
    for (int k = n; k <= IXW; ++k) {   // (offsets past the last window: its end)
        ab.b0[k] = bb;
        ar.b0[k] = br;
        ap.b0[k] = bp;
        ac.b0[k] = bc;
        an.b0[k] = 2 * n;
    }
    unsigned long long* dst = nullptr;
    uint64_t epoch = 0;
    MR_TRY(mr_dl_status(ctx, words, &dst, &epoch));
    DBuf<uint32_t> rows;   // (stream-ordered: freed back to this context's pool after the launches)
    DBuf<int8_t> side;
    MR_TRY(rows.alloc(ctx, (size_t)std::max<int64_t>(rwords, 1)));
    MR_TRY(side.alloc(ctx, (size_t)std::max<int64_t>(sbytes, 16)));
    for (int k = 0; k < n; ++k) {
        ab.w[k].rows = rows.p + roff[(size_t)k];
        ar.w[k].rows = rows.p + roff[(size_t)k];
        ab.w[k].side = side.p + soff[(size_t)k];
        ap.w[k].side = side.p + soff[(size_t)k];
        ar.w[k].side = side.p + soff[(size_t)k];
        {   // (the row of the traces in neither graph: the last of the window's zeroed words)
            const mr_spans* sp = sps[k];
            uint32_t* nr = zw[k] + 2 * ((int64_t)std::max(sp->lo_nk, 1) + 3 * (int64_t)sp->n_podops +
                                        std::max<int64_t>(sp->n_edge_keys, 1));
            ab.w[k].nrow = nr;
            ar.w[k].nrow = nr;
        }
        ap.w[k].st = dst + woff[(size_t)k];
    }
    hipLaunchKernelGGL(k_lo_build_b, dim3(bb), dim3(LB_T), lds, st, ab);
    hipLaunchKernelGGL(k_lo_pos_b, dim3(bp), dim3(LP_T), 0, st, ap, epoch);
    hipLaunchKernelGGL(k_lo_reduce_b, dim3(br), dim3(256), 0, st, ar);
    mr_ix_cross_nodes_launch(ctx, n, bc, ac, an);
    MR_TRY_HIP(ctx, hipGetLastError());
    for (int k = 0; k < n; ++k) g_lo_cmp_windows += cmps[(size_t)k] ? 1 : 0;   // (launched)
    return MR_OK;
}
