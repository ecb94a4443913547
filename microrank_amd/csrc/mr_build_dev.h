// What the graph-build units share (the library is built without relocatable device code, so a
// device function used by two units is defined here once, as in mr_pr_dev.h): the launch
// descriptors of a window's graph pair, the call-edge hash, and the one-block node order
// (nodes_small: get_pagerank_graph's node order, per-node arrays and P_ss,
// preprocess_data.py:159-171) that the indexed single-graph build (mr_build_ix.hip), the two-graph
// window batch (mr_build_win.hip) and the layout-order window batch (mr_build_lo.hip) all end in.
// The row-level build (mr_graph_build.hip) takes the hash and its constants.
#pragma once
#include "mr_detect_dev.h"
#include "mr_prim.h"

// ---------------------------------------------------------------- descriptors (host and device)
// nodes_small's arguments for one graph (a window's pair: block g builds graph g)
struct NsArgs {
    const uint32_t* gc;
    const int32_t *ocnt, *ofirst, *ocov;
    int32_t *node_of_code, *node_podop, *len_o, *nchild, *cov, *ss_par;
    int64_t* ss_off;
    const int64_t *T_dev, *nnz_dev;
    int64_t *rs_off, *out;
    float *u_o, *pw;   // (layout-order builds; else null)
    int32_t first_inv;  // (layout-order builds: ofirst holds INT_MAX - first row)
};
struct NsArgs2 {
    NsArgs g[2];
};
// A window's two graphs (online_rca.py:180,185: the detector's abnormal traces, state 2 -> graph 0
// "normal"; its normal traces, state 1 -> graph 1, T1) select disjoint traces of one table, so one
// pass over the per-trace index serves both: each entry goes to the graph of its trace's state.
// One graph's selection and counters:
struct IxSide {
    int32_t *tflag, *ocnt, *ofirst, *ocov;
    int64_t *tpos, *zoff;
    uint32_t* gc;
};
struct IxSide2 {
    IxSide g[2];
};
// a graph's trace rows and op lists (k_ix_traces' outputs)
struct TrOut {
    int32_t *trace_code, *len_t, *rs_ops;
    int64_t* rs_off;
    const int32_t* node_of_code;
};
struct TrOut2 {
    TrOut g[2];
};
// A chunk of windows (mr_windows_batch builds 4 per auxiliary stream) in ONE launch per stage
// instead of one per window: the per-window chains of ~6 small, latency-bound launches ran back
// to back on the stream (a C2 chunk: 24 launches before its read-back), now 6.  Per stage the
// windows' arguments travel by value; a block finds its window by the launch's block offsets
// (windows without blocks in a stage repeat the next offset) and works with its index inside the
// window.
constexpr int IXW = 8;   // windows per batched launch
template <class A>
struct IxBatch {
    int32_t n;
    int32_t b0[IXW + 1];
    A w[IXW];
};
// the two stages both window batches end in (mr_ix_cross_nodes_launch, mr_build_win.hip)
struct IxWinCross {
    const uint8_t* state;
    const int32_t *tc, *tp, *eid;
    int64_t n;
    IxSide2 x;
};
struct IxWinNodes {
    const uint64_t* gk;
    int64_t ecap;
    int32_t NP, pad_;
    NsArgs2 a;
};

// ---------------------------------------------------------------- device bodies
// (internal linkage, as in mr_pr_dev.h: a body's __shared__ arrays are private to the kernel it is
// inlined into)
namespace {
constexpr int ESET = 1024;         // per-block LDS edge set slots
constexpr uint64_t EMPTY = ~0ull;
__device__ __forceinline__ uint64_t hmix(uint64_t z) {
    z ^= z >> 33;
    z *= 0xff51afd7ed558ccdull;
    z ^= z >> 33;
    z *= 0xc4ceb9fe1a85ec53ull;
    return z ^ (z >> 33);
}
__device__ __forceinline__ void global_edge_add(uint64_t key, uint32_t c, uint64_t* gk, uint32_t* gc, uint64_t gmask) {
    uint64_t s = hmix(key) & gmask;
    for (;;) {
        unsigned long long k = atomicCAS((unsigned long long*)&gk[s], (unsigned long long)EMPTY, (unsigned long long)key);
        if (k == EMPTY || k == key) break;
        s = (s + 1) & gmask;
    }
    atomicAdd(&gc[s], c);
}
// ---------------------------------------------------------------- node order of a window graph, one block
// Windows (C2/C3: up to a few thousand pod-ops and call edges) take the whole of build_nodes in
// ONE single-block launch -- edges out of the hash table, parent flags and child counts, the
// node order (parents by code, the rest by first row, T10), per-node arrays, and P_ss by child --
// instead of ~15 launches and two host round trips.  Sizes go to `out` (N, E, overflow); a graph
// with more than NS_EMAX edges sets overflow and the caller runs build_nodes instead.
constexpr int NS_T = 1024, NS_PMAX = 4096, NS_EMAX = 8192;
static_assert(NS_EMAX <= 2 * NS_PMAX, "nodes_small: the CSR parents reuse the 64-bit key buffer");
__device__ __forceinline__ void ns_bitonic(uint64_t* a, int n) {   // n a power of two
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += NS_T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t x = a[i], y = a[ixj];
                    if ((x > y) == ((i & k) == 0)) {
                        a[i] = y;
                        a[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
}
// exclusive prefix of v over the block's threads (in thread order); total in *tot
__device__ __forceinline__ int32_t ns_scan(int32_t v, int32_t* sbuf, int32_t* tot) {
    sbuf[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < NS_T; o <<= 1) {
        const int32_t a = threadIdx.x >= o ? sbuf[threadIdx.x - o] : 0;
        __syncthreads();
        sbuf[threadIdx.x] += a;
        __syncthreads();
    }
    const int32_t incl = sbuf[threadIdx.x];
    if (threadIdx.x == NS_T - 1) *tot = incl;
    __syncthreads();
    return incl - v;
}
__device__ void nodes_small(const uint64_t* gk, const uint32_t* gc, int64_t ecap, const int32_t* ocnt,
                            const int32_t* ofirst, int32_t NP, int32_t* node_of_code, int32_t* node_podop,
                            int32_t* len_o, int32_t* nchild, const int32_t* ocov, int32_t* cov, int32_t* ss_par,
                            int64_t* ss_off, const int64_t* T_dev, const int64_t* nnz_dev, int64_t* rs_off,
                            int64_t* out, float* u_o = nullptr, float* pw = nullptr, bool first_inv = false) {
    __shared__ int32_t is_par[NS_PMAX], nch[NS_PMAX], noc[NS_PMAX];
    __shared__ uint64_t qb[NS_PMAX], eb[NS_EMAX];
    __shared__ int32_t sbuf[NS_T];
    __shared__ int32_t ecount, tot, P, Q;
    const int tid = threadIdx.x;
    for (int c = tid; c < NP; c += NS_T) {
        is_par[c] = 0;
        nch[c] = 0;
    }
    if (tid == 0) ecount = 0;
    __syncthreads();
    // call edges out of the hash table (parent code << 32 | child code): parents and child counts
    for (int64_t i = tid; i < ecap; i += NS_T) {
        const uint64_t k = gk[i];
        if (k == EMPTY || gc[i] == 0u) continue;   // (dense ids: a key of the table not in this graph)
        const int32_t par = (int32_t)(k >> 32);
        is_par[par] = 1;
        atomicAdd(&nch[par], (int32_t)gc[i]);
        const int32_t e = atomicAdd(&ecount, 1);
        if (e < NS_EMAX) eb[e] = k;
    }
    __syncthreads();
    const int32_t E = ecount;
    if (tid == 0) {   // the trace side's sizes (its scans ran before this launch)
        out[3] = *T_dev;
        out[4] = *nnz_dev;
        if (rs_off) rs_off[*T_dev] = *nnz_dev;
    }
    if (E > NS_EMAX) {
        if (tid == 0) out[2] = 1;
        return;
    }
    // node order: parents by code, then present non-parents by first row (T10)
    const int per = (NP + NS_T - 1) / NS_T, c0 = tid * per;   // each thread a run of codes
    int32_t np = 0, nq = 0;
    for (int c = c0; c < min(c0 + per, NP); ++c) {
        np += is_par[c] ? 1 : 0;
        nq += (!is_par[c] && ocnt[c] > 0) ? 1 : 0;
    }
    int32_t pp = ns_scan(np, sbuf, &tot);
    if (tid == 0) P = tot;
    __syncthreads();
    int32_t qp = ns_scan(nq, sbuf, &tot);
    if (tid == 0) Q = tot;
    __syncthreads();
    const int32_t nP = P, nQ = Q;
    for (int c = c0; c < min(c0 + per, NP); ++c) {
        if (is_par[c]) {
            noc[c] = pp;
            node_podop[pp] = c;
            ++pp;
        } else if (ocnt[c] > 0) {
            // (first_inv: the layout-order build keeps INT_MAX - first row, max-reduced)
            const int32_t fr = first_inv ? 0x7fffffff - ofirst[c] : ofirst[c];
            qb[qp++] = ((uint64_t)(uint32_t)fr << 32) | (uint32_t)c;
        }
    }
    __syncthreads();
    if (nQ <= NS_T) {   // rank of each (distinct) key by counting: one pass, no sorting network
        if (tid < nQ) {
            const uint64_t key = qb[tid];
            int32_t r = 0;
            for (int j = 0; j < nQ; ++j) r += qb[j] < key;
            const int32_t c = (int32_t)(key & 0xffffffffu);
            noc[c] = nP + r;
            node_podop[nP + r] = c;
        }
    } else {
        int qn = 1;
        while (qn < nQ) qn <<= 1;
        for (int i = nQ + tid; i < qn; i += NS_T) qb[i] = EMPTY;
        __syncthreads();
        ns_bitonic(qb, qn);
        for (int i = tid; i < nQ; i += NS_T) {
            const int32_t c = (int32_t)(qb[i] & 0xffffffffu);
            noc[c] = nP + i;
            node_podop[nP + i] = c;
        }
    }
    __syncthreads();
    const int32_t N = nP + nQ;
    for (int c = tid; c < NP; c += NS_T) node_of_code[c] = (is_par[c] || ocnt[c] > 0) ? noc[c] : -1;
    for (int c = c0; c < min(c0 + per, NP); ++c)   // per-node arrays (node_podop's writes are this block's)
        if (is_par[c] || ocnt[c] > 0) {
            len_o[noc[c]] = ocnt[c];
            nchild[noc[c]] = nch[c];
            cov[noc[c]] = ocov[c];
            if (u_o) {   // (layout-order builds: graph_consts' fp32 reciprocals, pagerank.py:39-52)
                u_o[noc[c]] = ocnt[c] > 0 ? (float)(1.0 / (double)ocnt[c]) : 0.0f;
                pw[noc[c]] = nch[c] > 0 ? (float)(1.0 / (double)nch[c]) : 0.0f;
            }
        }
    // P_ss by child (edges sorted by (child node, parent node)): a counting sort by child into
    // the CSR, then each child's few parents sorted in place.  (is_par / nch / qb are free now.)
    __syncthreads();
    int32_t* ccnt = nch;           // edges per child node
    int32_t* cpos = is_par;        // running insert position per child node
    int32_t* cpar = (int32_t*)qb;  // parents in CSR order (NS_EMAX <= 2 NS_PMAX slots)
    for (int n = tid; n < N; n += NS_T) ccnt[n] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += NS_T) {
        const uint64_t k = eb[e];
        const int32_t ch = noc[(int32_t)(k & 0xffffffffu)];
        eb[e] = ((uint64_t)(uint32_t)ch << 32) | (uint32_t)noc[(int32_t)(k >> 32)];
        atomicAdd(&ccnt[ch], 1);
    }
    __syncthreads();
    {
        const int perN = (N + NS_T - 1) / NS_T, n0 = tid * perN;
        int32_t run = 0;
        for (int n = n0; n < min(n0 + perN, N); ++n) run += ccnt[n];
        int32_t off = ns_scan(run, sbuf, &tot);
        for (int n = n0; n < min(n0 + perN, N); ++n) {
            cpos[n] = off;
            ss_off[n] = off;
            off += ccnt[n];
        }
        if (tid == 0) ss_off[N] = E;
    }
    __syncthreads();
    for (int e = tid; e < E; e += NS_T) {
        const uint64_t k = eb[e];
        cpar[atomicAdd(&cpos[(int32_t)(k >> 32)], 1)] = (int32_t)(k & 0xffffffffu);
    }
    __syncthreads();
    for (int n = tid; n < N; n += NS_T) {   // cpos[n] is now the end of child n's run
        const int32_t b = cpos[n], a = b - ccnt[n];
        for (int32_t i = a + 1; i < b; ++i) {   // insertion sort: runs are a child's few parents
            const int32_t v = cpar[i];
            int32_t j = i - 1;
            while (j >= a && cpar[j] > v) {
                cpar[j + 1] = cpar[j];
                --j;
            }
            cpar[j + 1] = v;
        }
    }
    __syncthreads();
    for (int e = tid; e < E; e += NS_T) ss_par[e] = cpar[e];
    if (tid == 0) {
        out[0] = N;
        out[1] = E;
        out[2] = 0;
    }
}
// ---------------------------------------------------------------- the index passes' shapes
constexpr int IX_EPT = 16;  // index entries per thread in k_ix_stats (fewer blocks: fewer global flushes)
// ... and in the window batches' k_ix_stats2_b for windows of >= IX_EPT_BIG index entries (C2's
// 2.3M, 256 windows per call: 16 / 64 -> 5752-5799 / 5926-5996 windows/s, profiles/r04ag); small
// windows (C3's 400k) keep 16: their blocks are few already
constexpr int IX_EPT_BATCH = 64;
constexpr int64_t IX_EPT_BIG = (int64_t)1 << 20;
// k_ix_stats: 16-wave blocks (one per CU) whose LDS holds the per-pod-op counts and first rows
// of up to IX_HIST codes (128 KB) beside the edge set: the C4 graph's 10k ops aggregate in LDS
// instead of a global atomic pair per index entry
constexpr int IX_BT = 1024;
constexpr int IX_HIST = 12288;   // three per-code counters (span count, first row, traces)
constexpr int IX_B = 8;     // entries per thread whose loads are batched
constexpr int64_t IX_LDS_WORDS = 36864;   // k_ix_stats' dynamic LDS budget (144 KB) in 4-B words
// the selection scans' tiles (k_ix_sel_scan, k_ix_sel_scan2_b): SEL_I traces per thread
constexpr int SEL_T = 256, SEL_I = 8, SEL_TILE = SEL_T * SEL_I;
// the graph of a detector state (T1 swap): 2 (abnormal) -> graph 0, 1 (normal) -> graph 1
__device__ __forceinline__ int side_of(uint8_t st) { return st == 2 ? 0 : st == 1 ? 1 : -1; }
// the window of this block in a batched launch
__device__ __forceinline__ int ixb_pick(const int32_t* b0, int32_t n) {
    const int32_t b = (int32_t)blockIdx.x;
    int k = 0;
    while (k + 1 < n && b0[k + 1] <= b) ++k;
    return k;
}
}  // namespace
