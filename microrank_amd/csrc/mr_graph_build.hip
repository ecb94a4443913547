// K1: preprocess_data.get_pagerank_graph (preprocess_data.py:146-171) on gfx950.
//
// From HBM-resident int-coded span columns and a trace mask (the trace_list, :148):
//   1. compact the selected rows, keeping row order (first appearance, T10)
//   2. per row: span counts per trace (len_t, :165) and per pod-op (len_o, :167), first
//      appearance row per pod-op, and the parent join ParentSpanId == spanID over the selected
//      rows regardless of traceID (preprocess_data.py:157-158, T11) -> distinct (parent op, child op) edges with
//      multiplicity (children multiset size, :159).  Hot keys (the root op is in every trace)
//      are aggregated in LDS per block before any global atomic.
//   3. node order: parent ops sorted by name (= code), then the other ops by first appearance
//      (preprocess_data.py:159-163, T10)
//   4. (trace, node) pairs -> stable radix sort -> distinct pairs = trace-major CSR (the
//      op-major side is derived by mr_graph_prepare as tiles); call edges sorted by
//      (child, parent) give P_ss by child.
//
// This unit: the graph entry points (mr_graph_build, mr_graph_build_sharded, mr_graph_nodes,
// mr_graph_export), the row-level build above (any span table; the last tier of the window build,
// win_detect_build in mr_detect.hip), build_nodes -- step 3 in its general multi-launch form,
// which the indexed build takes for sharded graphs and past the one-block limits -- and a sharded
// build's join across ranks.  The other builds, by stage: mr_build_ix.hip (one graph from the
// per-trace index), mr_build_win.hip (a window's two graphs in one index pass), mr_build_lo.hip
// (window graphs in layout order); what they share: mr_build_dev.h, mr_build_internal.h.
#include <algorithm>
#include <vector>

#include "mr_build_internal.h"
#include "mr_sort.h"

namespace {
constexpr int BT = 256;
constexpr int LDS_HIST = 8192;     // pod-op histograms in LDS up to this many codes

// ---------------------------------------------------------------- selection
// rows of masked traces; with a window (ts non-null) also inside it (the window's span_df)
__global__ void k_sel_flags(const int32_t* trace, int64_t S, const uint8_t* mask, const int64_t* ts, const int64_t* te,
                            int64_t t0, int64_t t1, int32_t* flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) flag[i] = (mask[trace[i]] && (!ts || (ts[i] >= t0 && te[i] <= t1))) ? 1 : 0;
}
__global__ void k_compact_rows(const int32_t* flag, const int64_t* pos, int64_t S, int32_t* rows) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S && flag[i]) rows[pos[i]] = (int32_t)i;
}

// ---------------------------------------------------------------- per-row statistics + join
__global__ void __launch_bounds__(BT) k_rows(const int32_t* rows, int64_t Ssel, const int32_t* trace,
                                             const int32_t* podop, const int64_t* parent, const int32_t* selflag,
                                             const int64_t* id_off, const int32_t* id_rows, int64_t n_codes,
                                             int32_t n_podops, int use_lds_hist, int32_t* tcnt, int32_t* ocnt,
                                             int32_t* ofirst, uint64_t* gk, uint32_t* gc, uint64_t gmask) {
    extern __shared__ int32_t lh[];   // [2*n_podops] counts, first rows (when use_lds_hist)
    __shared__ unsigned long long ek[ESET];
    __shared__ uint32_t ec[ESET];
    int32_t* lcnt = lh;
    int32_t* lfirst = lh + n_podops;
    if (use_lds_hist)
        for (int32_t i = threadIdx.x; i < n_podops; i += BT) {
            lcnt[i] = 0;
            lfirst[i] = 0x7fffffff;
        }
    for (int i = threadIdx.x; i < ESET; i += BT) {
        ek[i] = EMPTY;
        ec[i] = 0;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * BT * 8;
    for (int c = 0; c < 8; ++c) {
        const int64_t li = base + (int64_t)c * BT + threadIdx.x;   // local (selected) row index
        if (li >= Ssel) break;
        const int32_t r = rows[li];
        const int32_t op = podop[r];
        atomicAdd(&tcnt[trace[r]], 1);
        if (use_lds_hist) {
            atomicAdd(&lcnt[op], 1);
            atomicMin(&lfirst[op], (int32_t)li);
        } else {
            atomicAdd(&ocnt[op], 1);
            atomicMin(&ofirst[op], (int32_t)li);
        }
        const int64_t p = parent[r];
        if (p < 0 || p >= n_codes) continue;
        for (int64_t e = id_off[p]; e < id_off[p + 1]; ++e) {
            const int32_t j = id_rows[e];
            if (!selflag[j]) continue;
            const uint64_t key = ((uint64_t)(uint32_t)podop[j] << 32) | (uint32_t)op;   // (parent, child)
            uint32_t s = (uint32_t)(hmix(key) & (ESET - 1));
            bool done = false;
            for (int probe = 0; probe < 32; ++probe) {
                unsigned long long k = atomicCAS(&ek[s], (unsigned long long)EMPTY, (unsigned long long)key);
                if (k == EMPTY || k == key) {
                    atomicAdd(&ec[s], 1u);
                    done = true;
                    break;
                }
                s = (s + 1) & (ESET - 1);
            }
            if (!done) global_edge_add(key, 1u, gk, gc, gmask);   // LDS set crowded: go global
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ESET; i += BT)
        if (ek[i] != EMPTY) global_edge_add(ek[i], ec[i], gk, gc, gmask);
    if (use_lds_hist)
        for (int32_t i = threadIdx.x; i < n_podops; i += BT)
            if (lcnt[i]) {
                atomicAdd(&ocnt[i], lcnt[i]);
                atomicMin(&ofirst[i], lfirst[i]);
            }
}

// ---------------------------------------------------------------- node order
// a slot holds an edge when its key is set and counted (the dense form lists every key of the
// table, counted or not)
__global__ void k_edge_flags(const uint64_t* gk, const uint32_t* gc, int64_t cap, int32_t* flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) flag[i] = gk[i] != EMPTY && gc[i] != 0u;
}
__global__ void k_edge_compact(const uint64_t* gk, const uint32_t* gc, const int32_t* flag, const int64_t* pos,
                               int64_t cap, uint64_t* ekey, uint32_t* ecnt, int32_t* is_par, int32_t* nchild_code) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || !flag[i]) return;
    const uint64_t k = gk[i];
    ekey[pos[i]] = k;
    ecnt[pos[i]] = gc[i];
    const int32_t par = (int32_t)(k >> 32);
    is_par[par] = 1;
    atomicAdd(&nchild_code[par], (int32_t)gc[i]);
}
// flags: parent codes (sorted by code) and present non-parents keyed by first row
__global__ void k_node_flags(const int32_t* ocnt, const int32_t* is_par, int32_t n, int32_t* pflag, int32_t* qflag) {
    int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    pflag[c] = is_par[c] ? 1 : 0;
    qflag[c] = (ocnt[c] > 0 && !is_par[c]) ? 1 : 0;
}
__global__ void k_node_parents(const int32_t* pflag, const int64_t* ppos, const int32_t* qflag, const int64_t* qpos,
                               const int32_t* ofirst, int32_t n, int32_t* node_of_code, int32_t* node_podop,
                               uint64_t* qkey, uint32_t* qval) {
    int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    if (pflag[c]) {
        node_of_code[c] = (int32_t)ppos[c];
        node_podop[ppos[c]] = c;
    }
    if (qflag[c]) {
        qkey[qpos[c]] = (uint64_t)(uint32_t)ofirst[c];
        qval[qpos[c]] = (uint32_t)c;
    }
}
__global__ void k_node_rest(const uint32_t* qval, int64_t nq, int32_t P, int32_t* node_of_code, int32_t* node_podop) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int32_t c = (int32_t)qval[i];
    node_of_code[c] = P + (int32_t)i;
    node_podop[P + i] = c;
}

// ---------------------------------------------------------------- traces
__global__ void k_trace_flags(const int32_t* tcnt, int32_t n, int32_t* flag) {
    int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) flag[c] = tcnt[c] > 0;
}
__global__ void k_trace_index(const int32_t* flag, const int64_t* pos, const int32_t* tcnt, int32_t n,
                              int32_t* tidx_of_code, int32_t* trace_code, int32_t* len_t) {
    int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || !flag[c]) return;
    const int32_t t = (int32_t)pos[c];
    tidx_of_code[c] = t;
    trace_code[t] = c;
    len_t[t] = tcnt[c];
}

// ---------------------------------------------------------------- pairs
__global__ void k_pair_keys(const int32_t* rows, int64_t Ssel, const int32_t* trace, const int32_t* podop,
                            const int32_t* tidx_of_code, const int32_t* node_of_code, int nb, uint64_t* keys) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ssel) return;
    const int32_t r = rows[i];
    keys[i] = ((uint64_t)(uint32_t)tidx_of_code[trace[r]] << nb) | (uint32_t)node_of_code[podop[r]];
}
__global__ void k_run_heads(const uint64_t* keys, int64_t n, int32_t* flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}
// distinct pairs in (trace, node) order; every present trace has >= 1 pair, so its CSR offset is
// the position of its first pair (no per-trace counting atomics)
__global__ void k_pairs_out(const uint64_t* keys, const int32_t* flag, const int64_t* pos, int64_t n, int nb,
                            int64_t* rs_off, int32_t* rs_ops) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint64_t k = keys[i];
    const uint32_t t = (uint32_t)(k >> nb);
    const int64_t e = pos[i];
    rs_ops[e] = (int32_t)(k & ((1ull << nb) - 1));
    if (i == 0 || (keys[i - 1] >> nb) != t) rs_off[t] = e;
}
__global__ void k_set_last(int64_t* off, int32_t n, int64_t v) { off[n] = v; }

// ---------------------------------------------------------------- per-node arrays
__global__ void k_node_arrays(const int32_t* node_podop, int32_t N, const int32_t* ocnt, const int32_t* nchild_code,
                              const int32_t* ocov, int32_t* len_o, int32_t* nchild, int32_t* cov) {
    int32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int32_t c = node_podop[n];
    len_o[n] = ocnt[c];
    nchild[n] = nchild_code[c];
    if (ocov) cov[n] = ocov[c];
}
__global__ void k_edge_nodes(const uint64_t* ekey, int64_t E, const int32_t* node_of_code, int nb, uint64_t* skey) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const uint64_t k = ekey[i];
    const uint32_t par = (uint32_t)node_of_code[(int32_t)(k >> 32)];
    const uint32_t ch = (uint32_t)node_of_code[(int32_t)(k & 0xffffffffu)];
    skey[i] = ((uint64_t)ch << nb) | par;    // sort by (child, parent)
}
__global__ void k_edge_csr(const uint64_t* skey, int64_t E, int nb, int32_t* ss_par, int32_t* ccount) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    ss_par[i] = (int32_t)(skey[i] & ((1ull << nb) - 1));
    atomicAdd(&ccount[skey[i] >> nb], 1);
}

// ---------------------------------------------------------------- sharded build: the join across ranks
// A child row's parent rows may lie in traces of another rank (T11).  Each rank publishes a
// Bloom filter of the ParentSpanIds of its selected rows; a rank exports the selected rows whose
// spanID may be a parent on another rank (both filter bits set there); every rank joins its
// children against the other ranks' exports (exact spanID compare), counting edges at the child.
__device__ __forceinline__ uint32_t bloom_bit(uint64_t k, int i, int fb) {
    return (uint32_t)(hmix(k + (i ? 0x9E3779B97F4A7C15ull : 0ull)) >> 20) & ((1u << fb) - 1u);
}
__global__ void k_bloom_set(const int32_t* trace, const int64_t* parent, int64_t S, const uint8_t* mask, int fb,
                            uint32_t* F) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S || !mask[trace[i]] || parent[i] < 0) return;
    for (int h = 0; h < 2; ++h) {
        const uint32_t b = bloom_bit((uint64_t)parent[i], h, fb);
        atomicOr(&F[b >> 5], 1u << (b & 31));
    }
}
__global__ void k_export_flags(const int32_t* trace, const int64_t* span, int64_t S, const uint8_t* mask, int fb,
                               const uint32_t* Fall, int64_t words, int R, int me, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    int32_t hit = 0;
    if (mask[trace[i]]) {
        const uint32_t b0 = bloom_bit((uint64_t)span[i], 0, fb), b1 = bloom_bit((uint64_t)span[i], 1, fb);
        for (int r = 0; r < R && !hit; ++r) {
            if (r == me) continue;
            const uint32_t* F = Fall + (size_t)r * words;
            hit = ((F[b0 >> 5] >> (b0 & 31)) & (F[b1 >> 5] >> (b1 & 31)) & 1u) ? 1 : 0;
        }
    }
    flag[i] = hit;
}
// export record: (spanID code, pod-op | rank << 32); pads (~0, ~0) sort last
__global__ void k_export_fill(const int32_t* flag, const int64_t* pos, int64_t S, const int64_t* span,
                              const int32_t* podop, int me, int64_t cap, uint64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S && flag[i]) {
        out[2 * pos[i]] = (uint64_t)span[i];
        out[2 * pos[i] + 1] = (uint64_t)(uint32_t)podop[i] | ((uint64_t)(uint32_t)me << 32);
    }
    const int64_t n = pos[S];
    if (i >= n && i < cap) out[2 * i] = out[2 * i + 1] = ~0ull;
}
__global__ void k_export_keys(const uint64_t* rec, int64_t n, uint64_t* key, uint32_t* val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        key[i] = rec[2 * i];
        val[i] = (uint32_t)i;
    }
}
// per selected child row: the other ranks' export records with spanID == its parent
template <bool ADD>
__global__ void k_cross_join(const int32_t* trace, const int64_t* parent, const int32_t* podop, int64_t S,
                             const uint8_t* mask, const uint64_t* skey, const uint32_t* sval, const uint64_t* rec,
                             int64_t n, int me, unsigned long long* count, uint64_t* gk, uint32_t* gc, uint64_t gmask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S || !mask[trace[i]] || parent[i] < 0) return;
    const uint64_t p = (uint64_t)parent[i];
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    uint32_t c = 0;
    for (int64_t j = lo; j < n && skey[j] == p; ++j) {
        const uint64_t w = rec[2 * (size_t)sval[j] + 1];
        if ((int)(w >> 32) == me) continue;   // this rank's own rows: joined locally
        ++c;
        if (ADD) global_edge_add(((w & 0xffffffffull) << 32) | (uint32_t)podop[i], 1u, gk, gc, gmask);
    }
    if (!ADD && c) atomicAdd(count, (unsigned long long)c);
}
__global__ void k_neg_i32(int32_t* a, int32_t n) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = -a[i];
}
}  // namespace

static int read_i64(mr_ctx* ctx, const int64_t* dev, int64_t* host) { return mr_read_words(ctx, dev, 1, host); }

// Shared by the row-level and the indexed build (mr_build_ix.hip: sharded graphs, and graphs past
// the one-block limits), after the per-pod-op statistics and the call-edge hash are complete:
// call edges -> node order (sorted parent ops, then the others by first appearance, T10) ->
// per-node arrays (len_o, nchild) and P_ss by child.  ofirst holds a key per pod-op that orders
// first appearances like the DataFrame rows (row_bits wide).
// two int32 arrays of n cleared in one launch (instead of two memsets)
__global__ void k_zero2_i32(int32_t* a, int32_t* b, int32_t n) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        a[i] = 0;
        b[i] = 0;
    }
}
// sharded: node presence (span counts), first appearances and parent flags are reduced over the
// ranks for the node order (every rank the same N and order); len_o / nchild stay this rank's.
int mr_build_nodes(mr_ctx* ctx, mr_graph* g, int32_t NP, const int32_t* ocnt, const int32_t* ofirst, const int32_t* ocov,
                   int row_bits, const uint64_t* gk, const uint32_t* gc, uint64_t ecap, DBuf<int32_t>& node_of_code,
                   PhaseTimer* pt, bool sharded) {
    hipStream_t st = ctx->stream;
    DBuf<int32_t> eflag, is_par, nchild_code;
    DBuf<int64_t> epos, etmp, tmp;
    MR_TRY(eflag.alloc(ctx, ecap));
    MR_TRY(epos.alloc(ctx, ecap + 1));
    MR_TRY(etmp.alloc(ctx, scan_tmp_elems(ecap)));
    MR_TRY(tmp.alloc(ctx, std::max<int64_t>(scan_tmp_elems(NP), 1)));
    MR_TRY(is_par.alloc(ctx, NP));
    MR_TRY(nchild_code.alloc(ctx, NP));
    if (NP) hipLaunchKernelGGL(k_zero2_i32, dim3(cdiv(NP, 256)), dim3(256), 0, st, is_par.p, nchild_code.p, NP);
    hipLaunchKernelGGL(k_edge_flags, dim3(cdiv(ecap, 256)), dim3(256), 0, st, gk, gc, (int64_t)ecap, eflag.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, eflag.p, epos.p, ecap, etmp.p));
    int64_t E = 0;
    MR_TRY(read_i64(ctx, epos.p + ecap, &E));
    DBuf<uint64_t> ekey;
    DBuf<uint32_t> ecnt;
    MR_TRY(ekey.alloc(ctx, E));
    MR_TRY(ecnt.alloc(ctx, E));
    hipLaunchKernelGGL(k_edge_compact, dim3(cdiv(ecap, 256)), dim3(256), 0, st, gk, gc, eflag.p, epos.p, (int64_t)ecap,
                       ekey.p, ecnt.p, is_par.p, nchild_code.p);
    if (pt) pt->mark("edges");
    DBuf<int32_t> ocnt_g, ofirst_g;
    const int32_t* ocnt_o = ocnt;     // the node order's presence counts and first rows
    const int32_t* ofirst_o = ofirst;
    if (sharded && NP) {
        MR_TRY(ocnt_g.alloc(ctx, NP));
        MR_TRY(ofirst_g.alloc(ctx, NP));
        MR_TRY_HIP(ctx, hipMemcpyAsync(ocnt_g.p, ocnt, NP * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        MR_TRY_HIP(ctx, hipMemcpyAsync(ofirst_g.p, ofirst, NP * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_neg_i32, dim3(cdiv(NP, 256)), dim3(256), 0, st, ofirst_g.p, NP);
        MR_TRY(mr_coll_allreduce(ctx, is_par.p, NP, MR_DT_I32, 1));
        MR_TRY(mr_coll_allreduce(ctx, ocnt_g.p, NP, MR_DT_I32, 0));
        MR_TRY(mr_coll_allreduce(ctx, ofirst_g.p, NP, MR_DT_I32, 1));   // max of -first = min first
        hipLaunchKernelGGL(k_neg_i32, dim3(cdiv(NP, 256)), dim3(256), 0, st, ofirst_g.p, NP);
        ocnt_o = ocnt_g.p;
        ofirst_o = ofirst_g.p;
    }
    // node order
    DBuf<int32_t> pflag, qflag;
    DBuf<int64_t> ppos, qpos;
    MR_TRY(pflag.alloc(ctx, NP));
    MR_TRY(qflag.alloc(ctx, NP));
    MR_TRY(ppos.alloc(ctx, NP + 1));
    MR_TRY(qpos.alloc(ctx, NP + 1));
    MR_TRY(node_of_code.alloc(ctx, NP));
    if (NP) hipLaunchKernelGGL(k_node_flags, dim3(cdiv(NP, 256)), dim3(256), 0, st, ocnt_o, is_par.p, NP, pflag.p, qflag.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, pflag.p, ppos.p, NP, tmp.p));
    MR_TRY(mr_exclusive_scan_i32(ctx, qflag.p, qpos.p, NP, tmp.p));
    int64_t PQ[2] = {0, 0};
    MR_TRY_HIP(ctx, hipMemcpyAsync(&PQ[0], ppos.p + NP, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipMemcpyAsync(&PQ[1], qpos.p + NP, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    const int64_t P = PQ[0], Q = PQ[1];
    const int32_t N = (int32_t)(P + Q);
    MR_TRY(g->node_podop.alloc(ctx, N));
    DBuf<uint64_t> qkey;
    DBuf<uint32_t> qval;
    MR_TRY(qkey.alloc(ctx, Q));
    MR_TRY(qval.alloc(ctx, Q));
    if (NP)
        hipLaunchKernelGGL(k_node_parents, dim3(cdiv(NP, 256)), dim3(256), 0, st, pflag.p, ppos.p, qflag.p, qpos.p, ofirst_o,
                           NP, node_of_code.p, g->node_podop.p, qkey.p, qval.p);
    SortScratch ws;
    MR_TRY(mr_radix_sort(ctx, qkey.p, qval.p, Q, row_bits, ws));
    if (Q)
        hipLaunchKernelGGL(k_node_rest, dim3(cdiv(Q, 256)), dim3(256), 0, st, qval.p, Q, (int32_t)P, node_of_code.p,
                           g->node_podop.p);
    if (pt) pt->mark("order");
    // per-node arrays and P_ss
    const int nb = std::max(1, bits_for((uint64_t)std::max(N - 1, 0)));
    MR_TRY(g->len_o.alloc(ctx, N));
    MR_TRY(g->nchild.alloc(ctx, N));
    if (ocov) MR_TRY(g->cov.alloc(ctx, (size_t)std::max(N, 1)));
    if (N)
        hipLaunchKernelGGL(k_node_arrays, dim3(cdiv(N, 256)), dim3(256), 0, st, g->node_podop.p, N, ocnt, nchild_code.p,
                           ocov, g->len_o.p, g->nchild.p, g->cov.p);
    g->cov_ready = ocov != nullptr;
    DBuf<uint64_t> skey;
    MR_TRY(skey.alloc(ctx, E));
    if (E) hipLaunchKernelGGL(k_edge_nodes, dim3(cdiv(E, 256)), dim3(256), 0, st, ekey.p, E, node_of_code.p, nb, skey.p);
    MR_TRY(mr_radix_sort(ctx, skey.p, nullptr, E, 2 * nb, ws));
    DBuf<int32_t> ccount;
    DBuf<int64_t> ntmp;
    MR_TRY(ccount.zero(ctx, N));
    MR_TRY(ntmp.alloc(ctx, scan_tmp_elems(std::max(N, 1))));
    MR_TRY(g->ss_par.alloc(ctx, E));
    MR_TRY(g->ss_off.alloc(ctx, N + 1));
    if (E) hipLaunchKernelGGL(k_edge_csr, dim3(cdiv(E, 256)), dim3(256), 0, st, skey.p, E, nb, g->ss_par.p, ccount.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, ccount.p, g->ss_off.p, N, ntmp.p));
    MR_TRY_HIP(ctx, hipGetLastError());
    g->N = N;
    g->E = E;
    return MR_OK;
}

// Row-level build: any span table (rows selected by trace mask and, when `win`, by the
// trace-level time window of each row).
static int graph_build_rows(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, const int64_t* win, mr_graph* g) {
    hipStream_t st = ctx->stream;
    const int64_t S = sp->S;
    const int32_t NT = sp->n_traces, NP = sp->n_podops;
    // 1. selected rows
    DBuf<int32_t> selflag, rows;
    DBuf<int64_t> pos, tmp;
    const int64_t tmpn = std::max<int64_t>({scan_tmp_elems(S), scan_tmp_elems(NT), scan_tmp_elems(NP), 1});
    MR_TRY(selflag.alloc(ctx, S));
    MR_TRY(pos.alloc(ctx, S + 1));
    MR_TRY(tmp.alloc(ctx, tmpn));
    if (S)
        hipLaunchKernelGGL(k_sel_flags, dim3(cdiv(S, 256)), dim3(256), 0, st, sp->trace.p, S, d_mask, win ? sp->tstart.p : nullptr,
                           win ? sp->tend.p : nullptr, win ? win[0] : 0, win ? win[1] : 0, selflag.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, selflag.p, pos.p, S, tmp.p));
    int64_t Ssel = 0;
    MR_TRY(read_i64(ctx, pos.p + S, &Ssel));
    MR_TRY(rows.alloc(ctx, Ssel));
    if (S) hipLaunchKernelGGL(k_compact_rows, dim3(cdiv(S, 256)), dim3(256), 0, st, selflag.p, pos.p, S, rows.p);
    // 2. statistics + join
    DBuf<int32_t> tcnt, ocnt, ofirst;
    MR_TRY(tcnt.zero(ctx, NT));
    MR_TRY(ocnt.zero(ctx, NP));
    MR_TRY(ofirst.alloc(ctx, NP));
    if (NP) MR_TRY_HIP(ctx, hipMemsetAsync(ofirst.p, 0x7f, NP * sizeof(int32_t), st));
    const uint64_t ecap = mr_edge_capacity(Ssel, NP);
    DBuf<uint64_t> gk;
    DBuf<uint32_t> gc;
    MR_TRY(gk.alloc(ctx, ecap));
    MR_TRY(gc.zero(ctx, ecap));
    MR_TRY_HIP(ctx, hipMemsetAsync(gk.p, 0xff, ecap * sizeof(uint64_t), st));
    const int use_lds = NP <= LDS_HIST;
    const size_t lds = use_lds ? 2 * (size_t)NP * sizeof(int32_t) : 0;
    if (Ssel)
        hipLaunchKernelGGL(k_rows, dim3(cdiv(Ssel, BT * 8)), dim3(BT), lds, st, rows.p, Ssel, sp->trace.p, sp->podop.p,
                           sp->parent.p, selflag.p, sp->id_off.p, sp->id_rows.p, sp->n_span_codes, NP, use_lds, tcnt.p,
                           ocnt.p, ofirst.p, gk.p, gc.p, ecap - 1);
    // 3. edges, node order, per-node arrays, P_ss
    DBuf<int32_t> node_of_code;
    MR_TRY(mr_build_nodes(ctx, g, NP, ocnt.p, ofirst.p, nullptr, bits_for((uint64_t)std::max<int64_t>(Ssel, 1)), gk.p,
                       gc.p, ecap, node_of_code));
    const int32_t N = g->N;
    // traces
    DBuf<int32_t> tflag, tidx_of_code;
    DBuf<int64_t> tpos;
    MR_TRY(tflag.alloc(ctx, NT));
    MR_TRY(tpos.alloc(ctx, NT + 1));
    MR_TRY(tidx_of_code.alloc(ctx, NT));
    if (NT) hipLaunchKernelGGL(k_trace_flags, dim3(cdiv(NT, 256)), dim3(256), 0, st, tcnt.p, NT, tflag.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, tflag.p, tpos.p, NT, tmp.p));
    int64_t T64 = 0;
    MR_TRY(read_i64(ctx, tpos.p + NT, &T64));
    const int32_t T = (int32_t)T64;
    MR_TRY(g->trace_code.alloc(ctx, T));
    MR_TRY(g->len_t.alloc(ctx, T));
    if (NT)
        hipLaunchKernelGGL(k_trace_index, dim3(cdiv(NT, 256)), dim3(256), 0, st, tflag.p, tpos.p, tcnt.p, NT,
                           tidx_of_code.p, g->trace_code.p, g->len_t.p);
    // 4. pairs -> trace-major CSR
    const int nb = std::max(1, bits_for((uint64_t)std::max(N - 1, 0)));
    DBuf<uint64_t> keys;
    MR_TRY(keys.alloc(ctx, Ssel));
    if (Ssel)
        hipLaunchKernelGGL(k_pair_keys, dim3(cdiv(Ssel, 256)), dim3(256), 0, st, rows.p, Ssel, sp->trace.p, sp->podop.p,
                           tidx_of_code.p, node_of_code.p, nb, keys.p);
    SortScratch ws;
    MR_TRY(mr_radix_sort(ctx, keys.p, nullptr, Ssel, nb + bits_for((uint64_t)std::max(T - 1, 0)), ws));
    DBuf<int32_t> head;
    DBuf<int64_t> hpos;
    MR_TRY(head.alloc(ctx, Ssel));
    MR_TRY(hpos.alloc(ctx, Ssel + 1));
    if (Ssel) hipLaunchKernelGGL(k_run_heads, dim3(cdiv(Ssel, 256)), dim3(256), 0, st, keys.p, Ssel, head.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, head.p, hpos.p, Ssel, tmp.p));
    int64_t nnz = 0;
    MR_TRY(read_i64(ctx, hpos.p + Ssel, &nnz));
    MR_TRY(g->rs_ops.alloc(ctx, nnz));
    MR_TRY(g->rs_off.alloc(ctx, T + 1));
    if (Ssel)
        hipLaunchKernelGGL(k_pairs_out, dim3(cdiv(Ssel, 256)), dim3(256), 0, st, keys.p, head.p, hpos.p, Ssel, nb,
                           g->rs_off.p, g->rs_ops.p);
    mr_set_last(ctx, g->rs_off.p, T, nnz);
    MR_TRY_HIP(ctx, hipGetLastError());
    g->T = T;
    g->nnz_sr = g->nnz_rs = nnz;
    return MR_OK;
}

// The sharded build's cross-rank exchange (see k_bloom_set): the other ranks' export records
// sorted by spanID (keys / record index) and the number of cross-rank (child, parent) matches.
int mr_cross_exchange(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, CrossJoin& X) {
    hipStream_t st = ctx->stream;
    const int64_t S = sp->S;
    const int R = ctx->nranks, me = ctx->rank;
    DBuf<int64_t> sc;
    int64_t h = S;
    MR_TRY(sc.upload(ctx, &h, 1));
    MR_TRY(mr_coll_allreduce(ctx, sc.p, 1, MR_DT_I64, 1));   // the largest shard sizes the filters
    MR_TRY(sc.download(ctx, &h, 1));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    const int fb = std::min(28, std::max(16, bits_for((uint64_t)std::max<int64_t>(h, 1)) + 4));   // >= 16 bits per row
    const int64_t words = ((int64_t)1 << fb) / 32;
    DBuf<uint32_t> F, Fall;
    MR_TRY(F.zero(ctx, (size_t)words));
    MR_TRY(Fall.alloc(ctx, (size_t)words * R));
    if (S) hipLaunchKernelGGL(k_bloom_set, dim3(cdiv(S, 256)), dim3(256), 0, st, sp->trace.p, sp->parent.p, S, d_mask, fb, F.p);
    MR_TRY(mr_coll_allgather(ctx, F.p, Fall.p, words, MR_DT_I32));
    DBuf<int32_t> flag;
    DBuf<int64_t> pos, tmp;
    MR_TRY(flag.alloc(ctx, (size_t)std::max<int64_t>(S, 1)));
    MR_TRY(pos.alloc(ctx, (size_t)S + 1));
    MR_TRY(tmp.alloc(ctx, (size_t)std::max<int64_t>(scan_tmp_elems(S), 1)));
    if (S)
        hipLaunchKernelGGL(k_export_flags, dim3(cdiv(S, 256)), dim3(256), 0, st, sp->trace.p, sp->span.p, S, d_mask, fb,
                           Fall.p, words, R, me, flag.p);
    MR_TRY(mr_exclusive_scan_i32(ctx, flag.p, pos.p, S, tmp.p));
    MR_TRY_HIP(ctx, hipMemcpyAsync(sc.p, pos.p + S, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    MR_TRY(mr_coll_allreduce(ctx, sc.p, 1, MR_DT_I64, 1));   // the largest export list sizes the gather
    MR_TRY(sc.download(ctx, &h, 1));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    const int64_t cap = std::max<int64_t>(h, 1);
    DBuf<uint64_t> send;
    MR_TRY(send.alloc(ctx, 2 * (size_t)cap));
    hipLaunchKernelGGL(k_export_fill, dim3(cdiv(std::max<int64_t>(S, cap), 256)), dim3(256), 0, st, flag.p, pos.p, S,
                       sp->span.p, sp->podop.p, me, cap, send.p);
    X.n = cap * R;
    MR_TRY(X.rec.alloc(ctx, 2 * (size_t)X.n));
    MR_TRY(mr_coll_allgather(ctx, send.p, X.rec.p, 2 * cap, MR_DT_U64));
    MR_TRY(X.key.alloc(ctx, (size_t)X.n));
    MR_TRY(X.val.alloc(ctx, (size_t)X.n));
    hipLaunchKernelGGL(k_export_keys, dim3(cdiv(X.n, 256)), dim3(256), 0, st, X.rec.p, X.n, X.key.p, X.val.p);
    SortScratch ws;
    MR_TRY(mr_radix_sort(ctx, X.key.p, X.val.p, X.n, 64, ws));
    DBuf<unsigned long long> cnt;
    MR_TRY(cnt.zero(ctx, 1));
    if (S)
        hipLaunchKernelGGL(k_cross_join<false>, dim3(cdiv(S, 256)), dim3(256), 0, st, sp->trace.p, sp->parent.p,
                           sp->podop.p, S, d_mask, X.key.p, X.val.p, X.rec.p, X.n, me, cnt.p, (uint64_t*)nullptr,
                           (uint32_t*)nullptr, (uint64_t)0);
    unsigned long long m = 0;
    MR_TRY(cnt.download(ctx, &m, 1));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    X.matches = (int64_t)m;
    return MR_OK;
}

// the cross-rank parent joins into a build's edge hash, counted at the child's rank
int mr_cross_join_add(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, const CrossJoin& X, uint64_t* gk,
                      uint32_t* gc, uint64_t gmask) {
    if (X.matches && sp->S)
        hipLaunchKernelGGL(k_cross_join<true>, dim3(cdiv(sp->S, 256)), dim3(256), 0, ctx->stream, sp->trace.p,
                           sp->parent.p, sp->podop.p, sp->S, d_mask, X.key.p, X.val.p, X.rec.p, X.n, ctx->rank,
                           (unsigned long long*)nullptr, gk, gc, gmask);
    return MR_OK;
}

void mr_set_last(mr_ctx* ctx, int64_t* off, int32_t n, int64_t v) {
    hipLaunchKernelGGL(k_set_last, dim3(1), dim3(1), 0, ctx->stream, off, n, v);
}

// a built graph's trace-role fields and derived arrays (the K1 result is P_rs = P_sr)
int mr_graph_post_build(mr_ctx* ctx, mr_graph* g) {
    g->rs_is_sr = true;
    g->pr_identity = true;
    g->n_pr = g->T;
    PhaseTimer pt(ctx->stream, "prepare");
    MR_TRY(mr_graph_prepare(ctx, g));
    pt.mark("done");
    return MR_OK;
}

// win (nullable): [t0, t1] restricts rows to the time window on the row-level path; the indexed
// path is taken only when the window selects whole traces (uniform trace times) or is absent.
int mr_graph_build_dev(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, mr_graph** out, const int64_t* win) {
    auto g = new mr_graph();
    g->ctx = ctx;
    static const bool no_index = getenv("MR_NO_INDEX") != nullptr;   // A/B knob: force the row-level path
    const bool indexed = sp->indexed && !no_index && (!win || sp->uniform_times);
    int rc = indexed ? mr_graph_build_indexed(ctx, sp, d_mask, g) : graph_build_rows(ctx, sp, d_mask, win, g);
    if (rc == MR_OK) rc = mr_graph_post_build(ctx, g);
    if (rc != MR_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return MR_OK;
}

extern "C" int mr_graph_build(mr_ctx* ctx, const mr_spans* sp, const uint8_t* trace_mask, mr_graph** out) {
    if (!ctx || !sp || !trace_mask || !out || sp->ctx != ctx) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_build: bad arguments");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    DBuf<uint8_t> mask;
    MR_TRY(mask.upload(ctx, trace_mask, (size_t)sp->n_traces));
    MR_TRY(mr_graph_build_dev(ctx, sp, mask.p, out, nullptr));
    mr_handle_add(ctx, *out, [](void* h) { delete (mr_graph*)h; });
    return MR_OK;
}

extern "C" int mr_graph_build_sharded(mr_ctx* ctx, const mr_spans* sp, const uint8_t* trace_mask, mr_graph** out) {
    if (!ctx || !sp || !trace_mask || !out || sp->ctx != ctx)
        return mr_fail(ctx, MR_ERR_ARG, "mr_graph_build_sharded: bad arguments");
    if (!mr_coll_ready(ctx) && ctx->nranks != 1) return mr_fail(ctx, MR_ERR_COMM, "no collective backend");
    if (!sp->indexed) return mr_fail(ctx, MR_ERR_STATE, "span table has no per-trace index (sharded build needs it)");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    DBuf<uint8_t> mask;
    MR_TRY(mask.upload(ctx, trace_mask, (size_t)sp->n_traces));
    auto g = new mr_graph();
    g->ctx = ctx;
    g->shard_built = true;
    int rc = mr_graph_build_indexed(ctx, sp, mask.p, g, true);
    if (rc == MR_OK) {
        g->rs_is_sr = true;
        g->pr_identity = true;
        g->n_pr = g->T;
        rc = mr_graph_prepare(ctx, g);
    }
    if (rc == MR_OK) rc = hipStreamSynchronize(ctx->stream) == hipSuccess ? MR_OK : mr_fail(ctx, MR_ERR_HIP, "sync");
    if (rc != MR_OK) {
        delete g;
        return rc;
    }
    mr_handle_add(ctx, g, [](void* h) { delete (mr_graph*)h; });
    *out = g;
    return MR_OK;
}

extern "C" int mr_graph_nodes(const mr_graph* g, int32_t* node_podop, int32_t* trace_code) {
    if (!g) return MR_ERR_ARG;
    mr_ctx* ctx = g->ctx;
    if (!g->node_podop.p && g->N) return mr_fail(ctx, MR_ERR_STATE, "graph was not built from spans");
    if (node_podop && g->N) MR_TRY(g->node_podop.download(ctx, node_podop, g->N));
    if (trace_code && g->T) MR_TRY(g->trace_code.download(ctx, trace_code, g->T));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MR_OK;
}

extern "C" int mr_graph_export(const mr_graph* g, int64_t* sr_off, int32_t* sr_ops, int32_t* len_t, int32_t* len_o,
                               int64_t* ss_off, int32_t* ss_par, int32_t* nchild) {
    if (!g) return MR_ERR_ARG;
    mr_ctx* ctx = g->ctx;
    if (sr_off) MR_TRY(g->rs_off.download(ctx, sr_off, (size_t)g->T + 1));
    if (sr_ops) MR_TRY(g->rs_ops.download(ctx, sr_ops, (size_t)g->nnz_rs));
    if (sr_ops) {   // op lists in node order (the indexed build keeps pod-op code order)
        std::vector<int64_t> off((size_t)g->T + 1);
        MR_TRY(g->rs_off.download(ctx, off.data(), off.size()));
        MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int32_t t = 0; t < g->T; ++t) std::sort(sr_ops + off[t], sr_ops + off[t + 1]);
    }
    if (len_t) MR_TRY(g->len_t.download(ctx, len_t, (size_t)g->T));
    if (len_o) MR_TRY(g->len_o.download(ctx, len_o, (size_t)g->N));
    if (ss_off) MR_TRY(g->ss_off.download(ctx, ss_off, (size_t)g->N + 1));
    if (ss_par) MR_TRY(g->ss_par.download(ctx, ss_par, (size_t)g->E));
    if (nchild) MR_TRY(g->nchild.download(ctx, nchild, (size_t)g->N));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MR_OK;
}
