// The two-graph window batch: both graphs of each of n <= IXW windows (get_pagerank_graph twice
// per window, preprocess_data.py:146-171 through online_rca.py:180,185) from the detector's states
// in ONE pass over each table's per-trace index, a launch per stage for the whole chunk.  The
// second tier of the window build (win_chunk_build_async, mr_detect.hip): every table within
// mr_ix2_fits that has no layout order, and every table under MR_NO_LO_WIN.  Also here, behind
// mr_ix_cross_nodes_launch: the join-pair and node-order kernels that the layout-order batch
// (mr_build_lo.hip) ends in as well.
#include <algorithm>
#include <vector>

#include "mr_build_internal.h"

static_assert(SEL_T == 4 * WAVE, "k_ix_sel_scan2_b: one wave per look-back chain");
static_assert(DB == 4 * WAVE, "k_ix_detect_scan2_b: one wave per look-back chain");
// ---------------------------------------------------------------- per-window arguments of a stage
struct IxWinSel {
    DetIn d;   // (the detector-fused variant)
    const uint8_t* state;
    const int32_t* tlen;
    const int64_t* po_off;
    unsigned long long* st;   // this window's look-back status words (4 chains x its tiles)
    int64_t ecap;
    int32_t NT, NP;
    IxSide2 x;
};
struct IxWinStats {
    const uint8_t* state;
    const int32_t *po_tr, *po_op, *po_cnt, *po_first, *ed_tr, *ed_eid, *ed_cnt;
    int64_t n_po, n_ed;
    int32_t NP, n_ek;
    IxSide2 x;
};
struct IxWinTraces {
    const uint8_t* state;
    const int32_t *tlen, *po_tr, *po_op;
    const int64_t* po_off;
    int64_t n_po;
    int32_t NT, pad_;
    IxSide2 x;
    TrOut2 o;
};
// ---------------------------------------------------------------- stage bodies
// (blk_ of nblk_: the block's index among its window's.  Functions of internal linkage with their
// arguments by value: folded into their kernels they compile to other register, scratch and LDS
// allocations -- k_ix_detect_scan2_b to 49280 B of LDS for 41088.)
namespace {
// selection + the four exclusive scans (tpos and zoff of each graph) by decoupled look-back, and the
// clearing of both graphs' counters
__device__ __forceinline__ void ix_sel_scan2_body(const uint8_t* state, const int32_t* tlen, const int64_t* po_off,
                                                       int32_t NT, IxSide2 x, unsigned long long* st, uint64_t epoch,
                                                       int32_t NP, int64_t ecap, int32_t blk_, int32_t nblk_) {
    __shared__ int64_t sa[4][SEL_T];
    __shared__ int64_t ex[4];
    __shared__ int64_t so[SEL_TILE];   // the tile's outputs, staged for coalesced stores
    const int tid = threadIdx.x;
    const int64_t gsz = (int64_t)nblk_ * SEL_T, gi = (int64_t)blk_ * SEL_T + tid;
    for (int64_t i = gi; i < max((int64_t)NP, ecap); i += gsz)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (i < NP) {
                x.g[g].ocnt[i] = 0;
                x.g[g].ofirst[i] = 0x7f7f7f7f;
                x.g[g].ocov[i] = 0;
            }
            if (i < ecap) x.g[g].gc[i] = 0u;
        }
    const int64_t tile = blk_, t0 = tile * SEL_TILE, base = t0 + (int64_t)tid * SEL_I;
    int8_t sd[SEL_I];
    int64_t z[SEL_I], acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < SEL_I; ++i) {
        const int64_t t = base + i;
        const int s_ = t < NT && tlen[t] > 0 ? side_of(state[t]) : -1;
        sd[i] = (int8_t)s_;
        z[i] = s_ >= 0 ? po_off[t + 1] - po_off[t] : 0;
        if (s_ >= 0) {
            acc[2 * s_] += 1;
            acc[2 * s_ + 1] += z[i];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) sa[c][tid] = acc[c];
    __syncthreads();
    for (int o = 1; o < SEL_T; o <<= 1) {
        int64_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = tid >= o ? sa[c][tid - o] : 0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) sa[c][tid] += v[c];
        __syncthreads();
    }
    {   // wave c: chain c (graph c / 2, tpos or zoff)
        const int c = tid / WAVE;
        const int64_t agg = sa[c][SEL_T - 1];
        const int64_t e = dl_lookback_wave(st + (size_t)c * nblk_, tile, agg, epoch);
        if ((tid & (WAVE - 1)) == 0) {
            ex[c] = e;
            if (tile == (int64_t)nblk_ - 1) {
                int64_t* dst = (c & 1) ? x.g[c >> 1].zoff : x.g[c >> 1].tpos;
                dst[NT] = e + agg;
            }
        }
    }
    __syncthreads();
    // A thread's SEL_I values are consecutive traces: stored directly, each store instruction would
    // write 8 B into each of 64 lines (measured: 117 MB of WRITE_SIZE per 4-window chunk for 32 MB of
    // values); staged through LDS, every store is a coalesced run.  (Values of the graph a trace is
    // not in are never read.)
    int32_t* so32 = reinterpret_cast<int32_t*>(so);
#pragma unroll
    for (int i = 0; i < SEL_I; ++i) {   // both graphs' trace flags: halves of the stage
        so32[tid * SEL_I + i] = sd[i] == 0;
        so32[SEL_TILE + tid * SEL_I + i] = sd[i] == 1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SEL_I; ++k) {
        const int j = k * SEL_T + tid;
        if (t0 + j < NT) {
            x.g[0].tflag[t0 + j] = so32[j];
            x.g[1].tflag[t0 + j] = so32[SEL_TILE + j];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {   // c: graph c / 2, tpos (even) or zoff (odd)
        int64_t run = ex[c] + sa[c][tid] - acc[c];
        __syncthreads();   // (the previous round's stage has been read)
#pragma unroll
        for (int i = 0; i < SEL_I; ++i) {
            so[tid * SEL_I + i] = run;
            if (sd[i] == (c >> 1)) run += (c & 1) ? z[i] : 1;
        }
        __syncthreads();
        int64_t* dst = (c & 1) ? x.g[c >> 1].zoff : x.g[c >> 1].tpos;
#pragma unroll
        for (int k = 0; k < SEL_I; ++k) {
            const int j = k * SEL_T + tid;
            if (t0 + j < NT) dst[t0 + j] = so[j];
        }
    }
}
// The window's detector and k_ix_sel_scan2_b's selection scans in ONE launch: tiles of DB traces,
// each thread its trace's state (detect_block, into d.state for the later passes) and then the
// four look-back chains over one trace per thread.
__device__ __forceinline__ void ix_detect_scan2_body(DetIn d, const int64_t* po_off, int32_t NT, IxSide2 x,
                                                        unsigned long long* st, uint64_t epoch, int32_t NP,
                                                        int64_t ecap, int32_t blk_, int32_t nblk_) {
    __shared__ double term[DB * DCAP];
    __shared__ int64_t sa[4][DB];
    __shared__ int64_t ex[4];
    const int tid = threadIdx.x;
    const int64_t gsz = (int64_t)nblk_ * DB, gi = (int64_t)blk_ * DB + tid;
    for (int64_t i = gi; i < max((int64_t)NP, ecap); i += gsz)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (i < NP) {
                x.g[g].ocnt[i] = 0;
                x.g[g].ofirst[i] = 0x7f7f7f7f;
                x.g[g].ocov[i] = 0;
            }
            if (i < ecap) x.g[g].gc[i] = 0u;
        }
    const int stt = detect_block(NT, d, term, blk_);
    const int64_t tile = blk_, t = tile * DB + tid;
    const int s_ = t < NT && d.tlen[t] > 0 ? side_of((uint8_t)stt) : -1;
    const int64_t z = s_ >= 0 ? po_off[t + 1] - po_off[t] : 0;
    if (t < NT) {
        x.g[0].tflag[t] = s_ == 0;
        x.g[1].tflag[t] = s_ == 1;
    }
    int64_t acc[4] = {0, 0, 0, 0};
    if (s_ >= 0) {
        acc[2 * s_] = 1;
        acc[2 * s_ + 1] = z;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) sa[c][tid] = acc[c];
    __syncthreads();
    for (int o = 1; o < DB; o <<= 1) {
        int64_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = tid >= o ? sa[c][tid - o] : 0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) sa[c][tid] += v[c];
        __syncthreads();
    }
    {   // wave c: chain c (graph c / 2, tpos or zoff)
        const int c = tid / WAVE;
        const int64_t agg = sa[c][DB - 1];
        const int64_t e = dl_lookback_wave(st + (size_t)c * nblk_, tile, agg, epoch);
        if ((tid & (WAVE - 1)) == 0) {
            ex[c] = e;
            if (tile == (int64_t)nblk_ - 1) {
                int64_t* dst = (c & 1) ? x.g[c >> 1].zoff : x.g[c >> 1].tpos;
                dst[NT] = e + agg;
            }
        }
    }
    __syncthreads();
    if (t < NT) {   // (values of the graph the trace is not in are never read)
        x.g[0].tpos[t] = ex[0] + sa[0][tid] - acc[0];
        x.g[0].zoff[t] = ex[1] + sa[1][tid] - acc[1];
        x.g[1].tpos[t] = ex[2] + sa[2][tid] - acc[2];
        x.g[1].zoff[t] = ex[3] + sa[3][tid] - acc[3];
    }
}
// both graphs' per-pod-op counts / first rows / coverage and edge counts per dense id, one pass:
// block blk_ of the window's nblk_ takes a 1/nblk_ share of each list
__device__ __forceinline__ void ix_stats2_body(const uint8_t* state, int64_t n_po, const int32_t* po_tr,
                                                    const int32_t* po_op, const int32_t* po_cnt,
                                                    const int32_t* po_first, int64_t n_ed, const int32_t* ed_tr,
                                                    const int32_t* ed_eid, const int32_t* ed_cnt, int32_t NP,
                                                    int32_t n_ek, IxSide2 x, int32_t blk_, int32_t nblk_) {
    extern __shared__ int32_t lh[];
    const int32_t W = 3 * NP + n_ek;   // words per graph: cnt, first, cov, edge counts
    for (int32_t i = threadIdx.x; i < 2 * W; i += IX_BT) {
        const int32_t j = i % W;
        lh[i] = (j >= NP && j < 2 * NP) ? 0x7fffffff : 0;
    }
    __syncthreads();
    const int64_t pper = (n_po + nblk_ - 1) / nblk_, eper = (n_ed + nblk_ - 1) / nblk_;
    const int64_t p0 = (int64_t)blk_ * pper, p1 = min(p0 + pper, n_po);
    // (as k_ix_stats: a round's state gathers, then the next round's loads, then its atomics)
    int32_t tr[IX_B], op[IX_B], cn[IX_B], fr[IX_B];
    auto po_load = [&](int64_t rb) {
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            const int64_t r = min(rb + threadIdx.x + (int64_t)j * IX_BT, p1 - 1);
            tr[j] = po_tr[r];
            op[j] = po_op[r];
            cn[j] = po_cnt[r];
            fr[j] = po_first[r];
        }
    };
    if (p0 < p1) po_load(p0);
    for (int64_t rb = p0; rb < p1; rb += (int64_t)IX_BT * IX_B) {
        uint8_t sv[IX_B];
        int32_t cop[IX_B], ccn[IX_B], cfr[IX_B];
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            sv[j] = state[tr[j]];
            cop[j] = op[j];
            ccn[j] = cn[j];
            cfr[j] = fr[j];
        }
        if (rb + (int64_t)IX_BT * IX_B < p1) po_load(rb + (int64_t)IX_BT * IX_B);
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            const int sd = rb + threadIdx.x + (int64_t)j * IX_BT < p1 ? side_of(sv[j]) : -1;
            if (sd < 0) continue;
            int32_t* L = lh + sd * W;
            atomicAdd(&L[cop[j]], ccn[j]);
            atomicMin(&L[NP + cop[j]], cfr[j]);
            atomicAdd(&L[2 * NP + cop[j]], 1);
        }
    }
    const int64_t q0 = (int64_t)blk_ * eper, q1 = min(q0 + eper, n_ed);
    int32_t et[IX_B], ei[IX_B], en[IX_B];
    auto ed_load = [&](int64_t rb) {
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            const int64_t r = min(rb + threadIdx.x + (int64_t)j * IX_BT, q1 - 1);
            et[j] = ed_tr[r];
            ei[j] = ed_eid[r];
            en[j] = ed_cnt[r];
        }
    };
    if (q0 < q1) ed_load(q0);
    for (int64_t rb = q0; rb < q1; rb += (int64_t)IX_BT * IX_B) {
        uint8_t sv[IX_B];
        int32_t cid[IX_B], ccn[IX_B];
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            sv[j] = state[et[j]];
            cid[j] = ei[j];
            ccn[j] = en[j];
        }
        if (rb + (int64_t)IX_BT * IX_B < q1) ed_load(rb + (int64_t)IX_BT * IX_B);
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            const int sd = rb + threadIdx.x + (int64_t)j * IX_BT < q1 ? side_of(sv[j]) : -1;
            if (sd >= 0) atomicAdd((uint32_t*)&lh[sd * W + 3 * NP + cid[j]], (uint32_t)ccn[j]);
        }
    }
    __syncthreads();
    for (int32_t i = threadIdx.x; i < 2 * W; i += IX_BT) {
        const int32_t g = i / W, j = i % W;
        const int32_t v = lh[i];
        if (j < NP) {
            if (v) {
                atomicAdd(&x.g[g].ocnt[j], v);
                atomicMin(&x.g[g].ofirst[j], lh[g * W + NP + j]);
                atomicAdd(&x.g[g].ocov[j], lh[g * W + 2 * NP + j]);
            }
        } else if (j >= 3 * NP && v) {
            atomicAdd(&x.g[g].gc[j - 3 * NP], (uint32_t)v);
        }
    }
}
}  // namespace

// ---------------------------------------------------------------- kernels
// the detector on its own (windows not fused): each thread its trace's state, into d.state
__global__ void __launch_bounds__(DB) k_ix_detect_b(IxBatch<IxWinSel> a) {
    __shared__ double term[DB * DCAP];
    const int k = ixb_pick(a.b0, a.n);
    (void)detect_block(a.w[k].NT, a.w[k].d, term, (int32_t)blockIdx.x - a.b0[k]);
}
__global__ void __launch_bounds__(SEL_T) k_ix_sel_scan2_b(IxBatch<IxWinSel> a, uint64_t epoch) {
    const int k = ixb_pick(a.b0, a.n);
    const IxWinSel& w = a.w[k];
    ix_sel_scan2_body(w.state, w.tlen, w.po_off, w.NT, w.x, w.st, epoch, w.NP, w.ecap, (int32_t)blockIdx.x - a.b0[k],
                      a.b0[k + 1] - a.b0[k]);
}
__global__ void __launch_bounds__(DB) k_ix_detect_scan2_b(IxBatch<IxWinSel> a, uint64_t epoch) {
    const int k = ixb_pick(a.b0, a.n);
    const IxWinSel& w = a.w[k];
    ix_detect_scan2_body(w.d, w.po_off, w.NT, w.x, w.st, epoch, w.NP, w.ecap, (int32_t)blockIdx.x - a.b0[k],
                         a.b0[k + 1] - a.b0[k]);
}
__global__ void __launch_bounds__(IX_BT) k_ix_stats2_b(IxBatch<IxWinStats> a) {
    const int k = ixb_pick(a.b0, a.n);
    const IxWinStats& w = a.w[k];
    ix_stats2_body(w.state, w.n_po, w.po_tr, w.po_op, w.po_cnt, w.po_first, w.n_ed, w.ed_tr, w.ed_eid, w.ed_cnt, w.NP,
                   w.n_ek, w.x, (int32_t)blockIdx.x - a.b0[k], a.b0[k + 1] - a.b0[k]);
}
// join pairs across traces (T11): counted in a graph when both traces are in it
__global__ void k_ix_cross2_b(IxBatch<IxWinCross> a) {
    const int k = ixb_pick(a.b0, a.n);
    const IxWinCross& w = a.w[k];
    const int64_t i = (int64_t)((int32_t)blockIdx.x - a.b0[k]) * blockDim.x + threadIdx.x;
    if (i >= w.n) return;
    const int sd = side_of(w.state[w.tc[i]]);
    if (sd >= 0 && side_of(w.state[w.tp[i]]) == sd) atomicAdd(&w.x.g[sd].gc[w.eid[i]], 1u);
}
__global__ void __launch_bounds__(NS_T) k_nodes_small2_b(IxBatch<IxWinNodes> a) {   // block 2k + g: window k, graph g
    const int k = (int)blockIdx.x >> 1;
    const IxWinNodes& w = a.w[k];
    const NsArgs& x = w.a.g[blockIdx.x & 1];
    nodes_small(w.gk, x.gc, w.ecap, x.ocnt, x.ofirst, w.NP, x.node_of_code, x.node_podop, x.len_o, x.nchild, x.ocov, x.cov,
                x.ss_par, x.ss_off, x.T_dev, x.nnz_dev, x.rs_off, x.out, x.u_o, x.pw, x.first_inv != 0);
}
// both graphs' trace rows and op lists (k_ix_traces per graph)
__global__ void k_ix_traces2_b(IxBatch<IxWinTraces> a) {
    const int k = ixb_pick(a.b0, a.n);
    const IxWinTraces& w = a.w[k];
    const int64_t i = (int64_t)((int32_t)blockIdx.x - a.b0[k]) * blockDim.x + threadIdx.x;
    // (a trace is in graph sd iff its state's side is sd and it has rows -- the selection scan's
    // tflag, read from the state here: one gather less per entry; a trace with entries has rows)
    if (i < w.NT) {
        const int sd = side_of(w.state[i]);
        const int32_t len = w.tlen[i];
        if (sd >= 0 && len > 0) {
            const int32_t p = (int32_t)w.x.g[sd].tpos[i];
            w.o.g[sd].trace_code[p] = (int32_t)i;
            w.o.g[sd].len_t[p] = len;
            w.o.g[sd].rs_off[p] = w.x.g[sd].zoff[i];
        }
    }
    if (i < w.n_po) {
        const int32_t t = w.po_tr[i], op = w.po_op[i];
        const int sd = side_of(w.state[t]);
        if (sd >= 0) w.o.g[sd].rs_ops[w.x.g[sd].zoff[t] + (i - w.po_off[t])] = w.o.g[sd].node_of_code[op];
    }
}

// ---------------------------------------------------------------- host
void mr_ix_cross_nodes_launch(mr_ctx* ctx, int n, int32_t bc, const IxBatch<IxWinCross>& ac, const IxBatch<IxWinNodes>& an) {
    if (bc) hipLaunchKernelGGL(k_ix_cross2_b, dim3(bc), dim3(256), 0, ctx->stream, ac);
    hipLaunchKernelGGL(k_nodes_small2_b, dim3(2 * n), dim3(NS_T), 0, ctx->stream, an);
}

// Both graphs of each of n windows (1 <= n <= IXW; each: its table, state, graph pair, builds,
// size words -- those of graph j to d_outs[k] + 8 j) in five or six launches: the detector
// (k_ix_detect_b; fused into the next launch when `fuse`), selection and scans, statistics, join
// pairs across traces, node order, trace rows.  dets: the windows' detector inputs, their states
// written to d_states[k] (null: the states are given).
// MR_ERR_STATE: MR_NO_IX2 is set, or a window is outside the one-pass limits (mr_ix2_fits).  It is
// returned before the first allocation and the first launch: the caller's per-mask build runs the
// detector itself and starts from untouched builds and graphs.
int mr_ix_launch2_batch(mr_ctx* ctx, int n, const mr_spans* const* sps, uint8_t* const* d_states, mr_graph* const* g0s,
                        mr_graph* const* g1s, IxBuild* const* b0s, IxBuild* const* b1s, int64_t* const* d_outs,
                        const DetIn* dets, bool fuse) {
    if (n < 1 || n > IXW || getenv("MR_NO_IX2") != nullptr) return MR_ERR_STATE;
    for (int k = 0; k < n; ++k)
        if (!mr_ix2_fits(sps[k])) return MR_ERR_STATE;
    hipStream_t st = ctx->stream;
    IxBatch<IxWinSel> as{};
    IxBatch<IxWinStats> at{};
    const char* ee = getenv("MR_IX_EPT");   // (A/B knob, read per call)
    const int ept = ee ? std::max(1, atoi(ee)) : IX_EPT;   // (MR_IX_EPT forces it for every window)
    IxBatch<IxWinCross> ac{};
    IxBatch<IxWinNodes> an{};
    IxBatch<IxWinTraces> ar{};
    as.n = at.n = ac.n = an.n = ar.n = n;
    int32_t bs = 0, bt = 0, bc = 0, br = 0;
    size_t lds = 4;
    int64_t words = 0;
    std::vector<int64_t> woff((size_t)n);
    const int TP = fuse ? DB : SEL_TILE;   // traces per selection tile
    for (int k = 0; k < n; ++k) {
        const mr_spans* sp = sps[k];
        const int32_t NT = sp->n_traces, NP = sp->n_podops;
        const int64_t nek = sp->n_edge_keys;
        IxSide2 xs;
        NsArgs2 na;
        TrOut2 to;
        IxBuild* b[2] = {b0s[k], b1s[k]};
        mr_graph* g[2] = {g0s[k], g1s[k]};
        for (int j = 0; j < 2; ++j) {
            IxBuild& B = *b[j];
            mr_graph* G = g[j];
            B.dense = true;
            B.small = true;
            B.ecap = (uint64_t)nek;
            B.gkp = sp->ekey.p;
            MR_TRY(B.tflag.alloc(ctx, std::max(NT, 1)));
            MR_TRY(B.tpos.alloc(ctx, (size_t)NT + 1));
            MR_TRY(B.zoff.alloc(ctx, (size_t)NT + 1));
            MR_TRY(B.ocnt.alloc(ctx, std::max(NP, 1)));
            MR_TRY(B.ofirst.alloc(ctx, std::max(NP, 1)));
            MR_TRY(B.ocov.alloc(ctx, std::max(NP, 1)));
            MR_TRY(B.gc.alloc(ctx, (size_t)std::max<int64_t>(nek, 1)));
            IxSmall d;
            MR_TRY(mr_ix_small_buffers(ctx, sp, B, G, d_outs[k] + 8 * j, &d));
            xs.g[j] = d.x;
            na.g[j] = d.ns;
            to.g[j] = d.tr;
        }
        const int32_t nt = (int32_t)std::max<int64_t>(cdiv((int64_t)NT, TP), 1);
        woff[(size_t)k] = words;
        words += 4 * (int64_t)nt;
        as.b0[k] = bs;
        bs += nt;
        as.w[k] = IxWinSel{dets ? dets[k] : DetIn{}, d_states[k], sp->tlen.p, sp->po_off.p, nullptr, nek, NT, NP, xs};
        at.b0[k] = bt;
        const int64_t ne = std::max(sp->n_po, sp->n_ed);
        // (a window alone keeps IX_EPT: its blocks have the device to themselves -- 141 blocks of a C2
        // window against 36 at IX_EPT_BATCH; profiles/build_split/)
        const int ek = ee ? ept : n > 1 && ne >= IX_EPT_BIG ? IX_EPT_BATCH : IX_EPT;
        if (NT) bt += std::max(1, std::min(256, cdiv(ne, (int64_t)IX_BT * ek)));
        lds = std::max(lds, 2 * (3 * (size_t)NP + (size_t)nek) * sizeof(int32_t));
        at.w[k] = IxWinStats{d_states[k], sp->po_tr.p, sp->po_op.p, sp->po_cnt.p, sp->po_first.p, sp->ed_tr.p, sp->ed_eid.p,
                             sp->ed_cnt.p, sp->n_po, sp->n_ed, NP, (int32_t)nek, xs};
        ac.b0[k] = bc;
        bc += (int32_t)cdiv(sp->n_xj, 256);
        ac.w[k] = IxWinCross{d_states[k], sp->xj_tc.p, sp->xj_tp.p, sp->xj_eid.p, sp->n_xj, xs};
        an.b0[k] = 2 * k;
        an.w[k] = IxWinNodes{sp->ekey.p, nek, NP, 0, na};
        ar.b0[k] = br;
        if (NT || sp->n_po) br += (int32_t)cdiv(std::max<int64_t>(NT, sp->n_po), 256);
        ar.w[k] = IxWinTraces{d_states[k], sp->tlen.p, sp->po_tr.p, sp->po_op.p, sp->po_off.p, sp->n_po, NT, 0, xs, to};
    }
    for (int k = n; k <= IXW; ++k) {   // (offsets past the last window: its end)
        as.b0[k] = bs;
        at.b0[k] = bt;
        ac.b0[k] = bc;
        an.b0[k] = 2 * n;
        ar.b0[k] = br;
    }
    unsigned long long* dst = nullptr;
    uint64_t epoch = 0;
    MR_TRY(mr_dl_status(ctx, words, &dst, &epoch));
    for (int k = 0; k < n; ++k) as.w[k].st = dst + woff[(size_t)k];
    if (fuse) {
        hipLaunchKernelGGL(k_ix_detect_scan2_b, dim3(bs), dim3(DB), 0, st, as, epoch);
    } else {
        if (dets) {
            int32_t bd = 0;   // the detector's own launch: DB traces per block
            IxBatch<IxWinSel> ad = as;
            for (int k = 0; k < n; ++k) {
                ad.b0[k] = bd;
                bd += (int32_t)cdiv((int64_t)sps[k]->n_traces, DB);
            }
            for (int k = n; k <= IXW; ++k) ad.b0[k] = bd;
            if (bd) hipLaunchKernelGGL(k_ix_detect_b, dim3(bd), dim3(DB), 0, st, ad);
        }
        hipLaunchKernelGGL(k_ix_sel_scan2_b, dim3(bs), dim3(SEL_T), 0, st, as, epoch);
    }
    if (bt) hipLaunchKernelGGL(k_ix_stats2_b, dim3(bt), dim3(IX_BT), lds, st, at);
    mr_ix_cross_nodes_launch(ctx, n, bc, ac, an);
    if (br) hipLaunchKernelGGL(k_ix_traces2_b, dim3(br), dim3(256), 0, st, ar);
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;
}
