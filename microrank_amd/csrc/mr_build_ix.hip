// The indexed single-graph build: get_pagerank_graph (preprocess_data.py:146-171) for whole
// traces selected by a mask, every per-row fact taken from the per-trace index
// (mr_span_index.hip), so no row is sorted.  Each trace's op list is written in pod-op code order
// (a fixed order for the kind keys; mr_graph_export sorts by node id for inspection).
// It serves mr_graph_build / mr_graph_build_sharded and, in the window build
// (win_chunk_build_async, mr_detect.hip), the third tier: a build per mask for tables past the
// two-graph pass's limits or under MR_NO_IX2.  Also here: the buffers and descriptors of a graph
// that ends in the one-block node order, which both window batches take for each of their graphs.
#include <algorithm>
#include <cstring>

#include "mr_build_internal.h"

namespace {
// The indexed build's first launch: the trace selection with BOTH exclusive scans -- tpos over
// the selection flags, zoff over the selected traces' op-list lengths -- chained across tiles by
// decoupled look-back (two status chains), plus the clearing of the per-code counters and the
// edge hash (a grid-stride share per block): one launch where there were four.
__global__ void __launch_bounds__(SEL_T) k_ix_sel_scan(const uint8_t* mask, const int32_t* tlen, const int64_t* po_off,
                                                      int32_t NT, int32_t* tflag, int64_t* tpos, int64_t* zoff,
                                                      unsigned long long* st, uint64_t epoch, int32_t* ocnt,
                                                      int32_t* ofirst, int32_t* ocov, int32_t NP, uint64_t* gk,
                                                      uint32_t* gc, int64_t ecap) {
    __shared__ int64_t sa[SEL_T], sb[SEL_T];
    __shared__ int64_t ex[2];
    const int tid = threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * SEL_T, gi = (int64_t)blockIdx.x * SEL_T + tid;
    for (int64_t i = gi; i < max((int64_t)NP, ecap); i += gsz) {
        if (i < NP) {
            ocnt[i] = 0;
            ofirst[i] = 0x7f7f7f7f;   // larger than any row
            ocov[i] = 0;
        }
        if (i < ecap) {
            if (gk) gk[i] = ~0ull;
            gc[i] = 0u;
        }
    }
    const int64_t tile = blockIdx.x, base = tile * SEL_TILE + (int64_t)tid * SEL_I;
    int32_t f[SEL_I];
    int64_t z[SEL_I], a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < SEL_I; ++i) {
        const int64_t t = base + i;
        const bool on = t < NT && mask[t] && tlen[t] > 0;
        f[i] = on ? 1 : 0;
        z[i] = on ? po_off[t + 1] - po_off[t] : 0;
        if (t < NT) tflag[t] = f[i];
        a += f[i];
        b += z[i];
    }
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    for (int o = 1; o < SEL_T; o <<= 1) {
        const int64_t x = tid >= o ? sa[tid - o] : 0, y = tid >= o ? sb[tid - o] : 0;
        __syncthreads();
        sa[tid] += x;
        sb[tid] += y;
        __syncthreads();
    }
    if (tid < 2 * WAVE) {   // wave c: chain c
        const int c = tid / WAVE;
        const int64_t agg = c ? sb[SEL_T - 1] : sa[SEL_T - 1];
        const int64_t e = dl_lookback_wave(st + (size_t)c * gridDim.x, tile, agg, epoch);
        if ((tid & (WAVE - 1)) == 0) {
            ex[c] = e;
            if (tile == (int64_t)gridDim.x - 1) (c ? zoff : tpos)[NT] = e + agg;
        }
    }
    __syncthreads();
    int64_t ra = ex[0] + sa[tid] - a, rb = ex[1] + sb[tid] - b;
#pragma unroll
    for (int i = 0; i < SEL_I; ++i) {
        const int64_t t = base + i;
        if (t < NT) {
            tpos[t] = ra;
            zoff[t] = rb;
        }
        ra += f[i];
        rb += z[i];
    }
}
// Wide op spaces (more pod-op codes than one LDS histogram): the selected index entries of share b
// (the same 1/nblk shares k_ix_stats takes) grouped by op range of IX_HIST codes into out[p0, p1):
// a counting pass, then a scatter through wave-aggregated LDS cursors; tab[b (R + 1) + r] = the
// offset of range r in the share.  Each range's k_ix_stats blocks then read only their entries,
// once, instead of every range reading (and flag-checking) the whole index.
constexpr int IX_RMAX = 64;   // op ranges the grouping takes (786k codes)
__global__ void __launch_bounds__(IX_BT) k_ix_rpart(const int32_t* tflag, int64_t n_po, const int32_t* po_tr,
                                                 const int32_t* po_op, const int32_t* po_cnt, const int32_t* po_first,
                                                 int32_t nrange, int4* out, int32_t* tab) {
    __shared__ int32_t cnt[IX_RMAX], cur[IX_RMAX];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & (WAVE - 1);
    const int64_t pper = (n_po + gridDim.x - 1) / gridDim.x, p0 = (int64_t)blockIdx.x * pper, p1 = min(p0 + pper, n_po);
    if (tid < IX_RMAX) cnt[tid] = 0;
    __syncthreads();
    for (int64_t rb = p0; rb < p1; rb += IX_BT) {   // counts per range (a ballot per range present)
        const int64_t r = rb + tid;
        int32_t g = -1;
        if (r < p1 && tflag[po_tr[r]]) g = po_op[r] / IX_HIST;
        for (uint64_t todo = __ballot(g >= 0); todo;) {
            const int32_t q = __builtin_amdgcn_readlane(g, __ffsll((unsigned long long)todo) - 1);
            const uint64_t m = __ballot(g == q);
            if (lane == 0) atomicAdd(&cnt[q], __popcll(m));
            todo &= ~m;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int32_t a = 0;
        int32_t* tb = tab + (size_t)blockIdx.x * (nrange + 1);
        for (int q = 0; q < nrange; ++q) {
            cur[q] = a;
            tb[q] = a;
            a += cnt[q];
        }
        tb[nrange] = a;
    }
    __syncthreads();
    for (int64_t rb = p0; rb < p1; rb += IX_BT) {   // the scatter: one cursor add per range present
        const int64_t r = rb + tid;
        int32_t g = -1, op = 0, c = 0, f = 0;
        if (r < p1 && tflag[po_tr[r]]) {
            op = po_op[r];
            c = po_cnt[r];
            f = po_first[r];
            g = op / IX_HIST;
        }
        for (uint64_t todo = __ballot(g >= 0); todo;) {
            const int ld = __ffsll((unsigned long long)todo) - 1;
            const int32_t q = __builtin_amdgcn_readlane(g, ld);
            const uint64_t m = __ballot(g == q);
            int32_t base = 0;
            if (lane == ld) base = atomicAdd(&cur[q], __popcll(m));
            base = __builtin_amdgcn_readlane(base, ld);
            if (g == q) {
                const int32_t k = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                out[p0 + base + k] = make_int4(op - q * IX_HIST, c, f, 0);
            }
            todo &= ~m;
        }
    }
}
// entry-parallel over the index: span counts and first rows per pod-op of the selected traces
// (LDS-aggregated per block), and their join keys with multiplicity into the block's LDS edge
// set (hot keys aggregated before global atomics).  Block b takes a 1/gridDim share of each list.
__global__ void __launch_bounds__(IX_BT) k_ix_stats(const int32_t* tflag, int64_t n_po, const int32_t* po_tr,
                                                 const int32_t* po_op, const int32_t* po_cnt, const int32_t* po_first,
                                                 int64_t n_ed, const int32_t* ed_tr, const uint64_t* ed_key,
                                                 const int32_t* ed_cnt, int32_t n_podops, int use_lds_hist,
                                                 int32_t* ocnt, int32_t* ofirst, int32_t* ocov, uint64_t* gk,
                                                 uint32_t* gc, uint64_t gmask, const int32_t* ed_eid, int32_t n_ek,
                                                 int lds_ek, const int4* rent, const int32_t* rtab, int32_t nshare) {
    extern __shared__ int32_t lh[];
    __shared__ unsigned long long ek[ESET];
    __shared__ uint32_t ec[ESET];
    // more pod-op codes than one LDS histogram holds (wide op spaces, C5's 100k ops): blockIdx.x is an
    // op range of IX_HIST codes whose entries this block counts in LDS (the range's blocks share the
    // index: each reads its share of every entry and keeps those of its range); range 0 also takes
    // the join keys.  Was: three global atomics per entry at up to 10^5 codes.  blockIdx.y is the
    // share of the index.  rent: the share's selected entries grouped by range (k_ix_rpart) -- the
    // block reads only its range's.
    const int32_t rng = (int32_t)blockIdx.x, chunk = (int32_t)blockIdx.y, nchunk = (int32_t)gridDim.y;
    const int32_t op_lo = rng * IX_HIST;
    const bool ranged = gridDim.x > 1;
    const int32_t NPL = ranged ? min(IX_HIST, n_podops - op_lo) : n_podops;   // this block's codes
    n_podops = NPL;
    int32_t* lcnt = lh;
    int32_t* lfirst = lh + n_podops;
    int32_t* lcov = lh + 2 * n_podops;   // traces per pod-op (the graph's coverage)
    uint32_t* lec = (uint32_t*)(lh + (use_lds_hist ? 3 * n_podops : 0));   // dense edge ids: counts per id
    if (use_lds_hist)
        for (int32_t i = threadIdx.x; i < n_podops; i += IX_BT) {
            lcnt[i] = 0;
            lfirst[i] = 0x7fffffff;
            lcov[i] = 0;
        }
    if (ed_eid && lds_ek)
        for (int32_t i = threadIdx.x; i < n_ek; i += IX_BT) lec[i] = 0u;
    else if (!ed_eid)
        for (int i = threadIdx.x; i < ESET; i += IX_BT) {
            ek[i] = EMPTY;
            ec[i] = 0;
        }
    __syncthreads();
    const int64_t pper = (n_po + nchunk - 1) / nchunk, eper = (n_ed + nchunk - 1) / nchunk;
    // a round of IX_B entries per thread: its trace-flag gathers go out, then the NEXT round's loads,
    // then this round's atomics (the flags' wait leaves the younger loads in flight)
    const int64_t p0 = (int64_t)chunk * pper, p1 = min(p0 + pper, n_po);
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
    // (ranged: LDS histograms; this block's chunk = rpart's shares [s0, s1))
    const int32_t s0 = rent ? (int32_t)((int64_t)chunk * nshare / nchunk) : 0;
    const int32_t s1 = rent ? (int32_t)((int64_t)(chunk + 1) * nshare / nchunk) : 0;
    const int64_t sper = rent ? (n_po + nshare - 1) / nshare : 0;
    for (int32_t sh = s0; sh < s1; ++sh) {
        const int32_t* tb = rtab + (size_t)sh * (gridDim.x + 1);
        const int64_t e0 = sh * sper + tb[rng], e1 = sh * sper + tb[rng + 1];
        for (int64_t rb = e0; rb < e1; rb += (int64_t)IX_BT * IX_B) {
            int4 v[IX_B];
#pragma unroll
            for (int j = 0; j < IX_B; ++j) v[j] = rent[min(rb + threadIdx.x + (int64_t)j * IX_BT, e1 - 1)];
#pragma unroll
            for (int j = 0; j < IX_B; ++j) {
                if (rb + threadIdx.x + (int64_t)j * IX_BT >= e1) continue;
                atomicAdd(&lcnt[v[j].x], v[j].y);
                atomicMin(&lfirst[v[j].x], v[j].z);
                atomicAdd(&lcov[v[j].x], 1);
            }
        }
    }
    if (!rent && p0 < p1) po_load(p0);
    for (int64_t rb = p0; !rent && rb < p1; rb += (int64_t)IX_BT * IX_B) {
        int32_t fl[IX_B], cop[IX_B], ccn[IX_B], cfr[IX_B];
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            fl[j] = tflag[tr[j]];
            cop[j] = op[j] - op_lo;   // (0 unless ranged)
            ccn[j] = cn[j];
            cfr[j] = fr[j];
        }
        if (rb + (int64_t)IX_BT * IX_B < p1) po_load(rb + (int64_t)IX_BT * IX_B);
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            if (!(rb + threadIdx.x + (int64_t)j * IX_BT < p1 && (!ranged || (uint32_t)cop[j] < (uint32_t)NPL) && fl[j]))
                continue;
            if (use_lds_hist) {
                atomicAdd(&lcnt[cop[j]], ccn[j]);
                atomicMin(&lfirst[cop[j]], cfr[j]);
                atomicAdd(&lcov[cop[j]], 1);
            } else {
                atomicAdd(&ocnt[cop[j]], ccn[j]);
                atomicMin(&ofirst[cop[j]], cfr[j]);
                atomicAdd(&ocov[cop[j]], 1);
            }
        }
    }
    const int64_t q0 = (int64_t)chunk * eper, q1 = rng ? q0 : min(q0 + eper, n_ed);   // (range 0: the keys)
    if (ed_eid) {   // dense edge ids: one counter add per selected entry
        for (int64_t rb = q0; rb < q1; rb += (int64_t)IX_BT * IX_B) {
            int32_t tr[IX_B], cn[IX_B], id[IX_B];
#pragma unroll
            for (int j = 0; j < IX_B; ++j) {
                const int64_t r = min(rb + threadIdx.x + (int64_t)j * IX_BT, q1 - 1);
                tr[j] = ed_tr[r];
                id[j] = ed_eid[r];
                cn[j] = ed_cnt[r];
            }
#pragma unroll
            for (int j = 0; j < IX_B; ++j)
                if (rb + threadIdx.x + (int64_t)j * IX_BT < q1 && tflag[tr[j]]) {
                    if (lds_ek) atomicAdd(&lec[id[j]], (uint32_t)cn[j]);
                    else atomicAdd(&gc[id[j]], (uint32_t)cn[j]);
                }
        }
        __syncthreads();
        if (lds_ek)
            for (int32_t i = threadIdx.x; i < n_ek; i += IX_BT)
                if (lec[i]) atomicAdd(&gc[i], lec[i]);
        if (use_lds_hist)
            for (int32_t i = threadIdx.x; i < n_podops; i += IX_BT)
                if (lcnt[i]) {
                    atomicAdd(&ocnt[op_lo + i], lcnt[i]);
                    atomicMin(&ofirst[op_lo + i], lfirst[i]);
                    atomicAdd(&ocov[op_lo + i], lcov[i]);
                }
        return;
    }
    for (int64_t rb = q0; rb < q1; rb += (int64_t)IX_BT * IX_B) {
        int32_t tr[IX_B], cn[IX_B];
        uint64_t ky[IX_B];
        bool on[IX_B];
#pragma unroll
        for (int j = 0; j < IX_B; ++j) {
            const int64_t r = min(rb + threadIdx.x + (int64_t)j * IX_BT, q1 - 1);
            tr[j] = ed_tr[r];
            ky[j] = ed_key[r];
            cn[j] = ed_cnt[r];
        }
#pragma unroll
        for (int j = 0; j < IX_B; ++j) on[j] = rb + threadIdx.x + (int64_t)j * IX_BT < q1 && tflag[tr[j]];
        for (int j = 0; j < IX_B; ++j) {
            if (!on[j]) continue;
            const uint64_t key = ky[j];
            uint32_t s = (uint32_t)(hmix(key) & (ESET - 1));
            bool done = false;
            for (int probe = 0; probe < 32; ++probe) {
                unsigned long long kk = atomicCAS(&ek[s], (unsigned long long)EMPTY, (unsigned long long)key);
                if (kk == EMPTY || kk == key) {
                    atomicAdd(&ec[s], (uint32_t)cn[j]);
                    done = true;
                    break;
                }
                s = (s + 1) & (ESET - 1);
            }
            if (!done) global_edge_add(key, (uint32_t)cn[j], gk, gc, gmask);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ESET; i += IX_BT)
        if (ek[i] != EMPTY) global_edge_add(ek[i], ec[i], gk, gc, gmask);
    if (use_lds_hist)
        for (int32_t i = threadIdx.x; i < n_podops; i += IX_BT)
            if (lcnt[i]) {
                atomicAdd(&ocnt[op_lo + i], lcnt[i]);
                atomicMin(&ofirst[op_lo + i], lfirst[i]);
                atomicAdd(&ocov[op_lo + i], lcov[i]);
            }
}
// Edges counted in edge-id order (mr_spans.eb_*, large tables): a lane per entry, the wave's runs
// of one id summed by a segmented scan (ids ascend along the wave), a wave walking EC_CH chunks
// with the last run's sum carried from chunk to chunk, one add per run into cnt[id] -- in place of
// an atomic (or a hash probe) per entry, and a hot id (millions of entries) takes one add per
// 2048 entries, not per 64.  The selection is read from a
// bitmap of the traces (NT / 8 bytes: the gathers stay in L2).
__global__ void k_tbits(const int32_t* tflag, int32_t NT, uint64_t* bits) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = __ballot(t < NT && tflag[t] != 0);
    if ((threadIdx.x & (WAVE - 1)) == 0 && t < NT) bits[t >> 6] = m;
}
constexpr int EC_CH = 32;   // k_ix_ecount: chunks of 64 entries per wave (a run's sum carried across them)
__global__ void k_ix_ecount(const int32_t* eb_tr, const int32_t* eb_cnt, const int32_t* eb_eid, int64_t n,
                            const uint64_t* tb, uint32_t* cnt) {
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    int32_t ce = -1;   // the run that continues into the next chunk (wave-uniform) and its sum so far
    uint32_t cv = 0u;
    for (int c = 0; c < EC_CH; ++c) {
        const int64_t i = (w * EC_CH + c) * WAVE + lane;
        if (w * EC_CH * WAVE + (int64_t)c * WAVE >= n) break;   // (wave-uniform)
        const bool in = i < n;
        const int32_t e = in ? eb_eid[i] : -1;
        const int32_t t = in ? eb_tr[i] : 0;
        uint32_t v = (in && ((tb[t >> 6] >> (t & 63)) & 1ull)) ? (uint32_t)eb_cnt[i] : 0u;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {   // inclusive segmented scan (ids ascend along the wave)
            const uint32_t u = __shfl_up(v, o, WAVE);
            const int32_t eu = __shfl_up(e, o, WAVE);
            if (lane >= o && eu == e) v += u;
        }
        if (e == ce) v += cv;   // (the chunk's first run continues the carried one)
        else if (lane == 0 && ce >= 0 && cv) atomicAdd(&cnt[ce], cv);   // (or the carried run ended with the chunk)
        const int32_t en = __shfl_down(e, 1, WAVE);
        if (in && v && lane != WAVE - 1 && en != e) atomicAdd(&cnt[e], v);
        ce = __builtin_amdgcn_readlane(e, WAVE - 1);
        cv = (uint32_t)__builtin_amdgcn_readlane((int)v, WAVE - 1);
    }
    if (lane == 0 && ce >= 0 && cv) atomicAdd(&cnt[ce], cv);
}
// a sharded build's hash set from the per-id counts (one insert per id present, not per entry)
__global__ void k_ix_edense_hash(const uint64_t* ekey, const uint32_t* cnt, int64_t E, uint64_t* gk, uint32_t* gc,
                                 uint64_t gmask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E && cnt[i]) global_edge_add(ekey[i], cnt[i], gk, gc, gmask);
}
// join pairs whose rows lie in different traces count when both traces are selected (T11)
__global__ void k_ix_cross(const uint8_t* mask, const int32_t* tc, const int32_t* tp, const uint64_t* key, int64_t n,
                           uint64_t* gk, uint32_t* gc, uint64_t gmask, const int32_t* eid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && mask[tc[i]] && mask[tp[i]]) {
        if (eid) atomicAdd(&gc[eid[i]], 1u);
        else global_edge_add(key[i], 1u, gk, gc, gmask);
    }
}
// the selected traces' rows (trace_code, len_t, CSR offsets) and, entry-parallel, their op lists
// rs_ops[zoff[t] + k] = node of the k-th pod-op: one launch over max(NT, n_po)
__global__ void k_ix_traces(const int32_t* tflag, const int64_t* tpos, const int64_t* zoff, int32_t NT,
                            const int32_t* tlen, int32_t* trace_code, int32_t* len_t, int64_t* rs_off, int64_t n_po,
                            const int32_t* po_tr, const int64_t* po_off, const int32_t* po_op,
                            const int32_t* node_of_code, int32_t* rs_ops) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NT && tflag[i]) {
        const int32_t p = (int32_t)tpos[i];
        trace_code[p] = (int32_t)i;
        len_t[p] = tlen[i];
        rs_off[p] = zoff[i];
    }
    if (i < n_po) {
        const int32_t t = po_tr[i];
        if (tflag[t]) rs_ops[zoff[t] + (i - po_off[t])] = node_of_code[po_op[i]];
    }
}
__global__ void __launch_bounds__(NS_T) k_nodes_small(const uint64_t* gk, const uint32_t* gc, int64_t ecap,
                                                     const int32_t* ocnt, const int32_t* ofirst, int32_t NP,
                                                     int32_t* node_of_code, int32_t* node_podop, int32_t* len_o,
                                                     int32_t* nchild, const int32_t* ocov, int32_t* cov,
                                                     int32_t* ss_par, int64_t* ss_off, const int64_t* T_dev,
                                                     const int64_t* nnz_dev, int64_t* rs_off, int64_t* out) {
    nodes_small(gk, gc, ecap, ocnt, ofirst, NP, node_of_code, node_podop, len_o, nchild, ocov, cov, ss_par, ss_off,
                T_dev, nnz_dev, rs_off, out);
}
}  // namespace

int mr_ix_graph_buffers(mr_ctx* ctx, int32_t NP, IxBuild& B, mr_graph* G) {
    MR_TRY(B.node_of_code.alloc(ctx, std::max(NP, 1)));
    MR_TRY(G->node_podop.alloc(ctx, std::max(NP, 1)));
    MR_TRY(G->len_o.alloc(ctx, std::max(NP, 1)));
    MR_TRY(G->nchild.alloc(ctx, std::max(NP, 1)));
    MR_TRY(G->cov.alloc(ctx, std::max(NP, 1)));
    MR_TRY(G->ss_par.alloc(ctx, NS_EMAX));
    MR_TRY(G->ss_off.alloc(ctx, (size_t)NP + 1));
    return MR_OK;
}
int mr_ix_small_buffers(mr_ctx* ctx, const mr_spans* sp, IxBuild& B, mr_graph* G, int64_t* d_out, IxSmall* out) {
    const int32_t NT = sp->n_traces, NP = sp->n_podops;
    MR_TRY(mr_ix_graph_buffers(ctx, NP, B, G));
    MR_TRY(G->trace_code.alloc(ctx, std::max(NT, 1)));
    MR_TRY(G->len_t.alloc(ctx, std::max(NT, 1)));
    MR_TRY(G->rs_ops.alloc(ctx, (size_t)std::max<int64_t>(sp->n_po, 1)));
    MR_TRY(G->rs_off.alloc(ctx, (size_t)NT + 1));
    out->x = IxSide{B.tflag.p, B.ocnt.p, B.ofirst.p, B.ocov.p, B.tpos.p, B.zoff.p, B.gc.p};
    out->ns = NsArgs{B.gc.p, B.ocnt.p, B.ofirst.p, B.ocov.p, B.node_of_code.p, G->node_podop.p, G->len_o.p, G->nchild.p,
                     G->cov.p, G->ss_par.p, G->ss_off.p, B.tpos.p + NT, B.zoff.p + NT, G->rs_off.p, d_out, nullptr, nullptr};
    out->tr = TrOut{G->trace_code.p, G->len_t.p, G->rs_ops.p, G->rs_off.p, B.node_of_code.p};
    return MR_OK;
}
// the selected traces' rows and op lists into g, over b's selection and node_of_code
static void ix_traces_launch(mr_ctx* ctx, const mr_spans* sp, const IxBuild& b, mr_graph* g) {
    const int32_t NT = sp->n_traces;
    if (NT || sp->n_po)
        hipLaunchKernelGGL(k_ix_traces, dim3(cdiv(std::max<int64_t>(NT, sp->n_po), 256)), dim3(256), 0, ctx->stream,
                           b.tflag.p, b.tpos.p, b.zoff.p, NT, sp->tlen.p, g->trace_code.p, g->len_t.p, g->rs_off.p,
                           sp->n_po, sp->po_tr.p, sp->po_off.p, sp->po_op.p, b.node_of_code.p, g->rs_ops.p);
}

// Split in two so a caller can read the sizes of several builds (and other counters) in ONE host
// round trip: mr_ix_launch enqueues everything up to the one-block node order (sizes to d_out:
// N, E, overflow, T, nnz), mr_ix_finish takes them (h, or null: read here) and completes the
// graph -- on overflow / sharded graphs through the general node order.
static int ix_launch(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, mr_graph* g, IxBuild& b, int64_t* d_out,
                     bool sharded) {
    hipStream_t st = ctx->stream;
    const int32_t NT = sp->n_traces, NP = sp->n_podops;
    CrossJoin X;
    if (sharded && ctx->nranks > 1) MR_TRY(mr_cross_exchange(ctx, sp, d_mask, X));   // (one rank: all joins local)
    MR_TRY(b.tflag.alloc(ctx, NT));
    MR_TRY(b.tpos.alloc(ctx, NT + 1));
    MR_TRY(b.zoff.alloc(ctx, NT + 1));
    MR_TRY(b.ocnt.alloc(ctx, NP));
    MR_TRY(b.ofirst.alloc(ctx, NP));
    MR_TRY(b.ocov.alloc(ctx, NP));
    // dense edge ids (one table's keys, counted per id) unless joins across ranks bring keys the
    // table does not hold
    const bool no_dense = getenv("MR_EDGE_HASH") != nullptr;   // A/B knob (read per call: tests flip it)
    b.dense = !sharded && !no_dense && sp->ekey.p != nullptr;
    b.ecap = b.dense ? (uint64_t)sp->n_edge_keys : mr_edge_capacity(sp->n_edge_keys + X.matches, NP);
    const uint64_t ecap = b.ecap;
    if (!b.dense) MR_TRY(b.gk.alloc(ctx, ecap));
    MR_TRY(b.gc.alloc(ctx, std::max<uint64_t>(ecap, 1)));
    b.gkp = b.dense ? sp->ekey.p : b.gk.p;
    {   // selection + both trace scans + clearing, one launch
        const int64_t nt = std::max<int64_t>(cdiv((int64_t)NT, SEL_TILE), 1);
        unsigned long long* dst = nullptr;
        uint64_t epoch = 0;
        MR_TRY(mr_dl_status(ctx, 2 * nt, &dst, &epoch));
        hipLaunchKernelGGL(k_ix_sel_scan, dim3((unsigned)nt), dim3(SEL_T), 0, st, d_mask, sp->tlen.p, sp->po_off.p, NT,
                           b.tflag.p, b.tpos.p, b.zoff.p, dst, epoch, b.ocnt.p, b.ofirst.p, b.ocov.p, NP,
                           b.dense ? (uint64_t*)nullptr : b.gk.p, b.gc.p, (int64_t)ecap);
    }
    if (NT) {
        // more codes than one LDS histogram: op ranges of IX_HIST codes in blockIdx.y
        const int nrange = NP > IX_HIST ? cdiv(NP, IX_HIST) : 1;
        const int use_lds = NP <= IX_HIST || nrange > 1;
        const int64_t NPL = std::min<int64_t>(NP, IX_HIST);
        // dense edge counts in LDS beside the pod-op histogram while both fit (else global adds)
        const int lds_ek = b.dense && (use_lds ? 3 * NPL : 0) + (int64_t)ecap <= IX_LDS_WORDS;
        const size_t lds = (use_lds ? 3 * (size_t)NPL * sizeof(int32_t) : 0) + (lds_ek ? ecap * sizeof(uint32_t) : 0);
        constexpr int ix_cap = 256;   // block cap: one per CU
        int nblk = std::max(1, std::min(ix_cap, cdiv(std::max(sp->n_po, sp->n_ed), IX_BT * IX_EPT)));
        if (nrange > 1) nblk = std::max(1, std::min(nblk, 2 * ix_cap / nrange));   // ~2 rounds of one block per CU
        // ranged: the entries grouped by range first (k_ix_rpart over nshare shares, 4 blocks per CU)
        DBuf<int4> rent;
        DBuf<int32_t> rtab;
        int32_t nshare = 0;
        if (nrange > 1 && nrange <= IX_RMAX && sp->n_po > 0) {
            nshare = (int32_t)std::max<int64_t>(nblk, std::min<int64_t>(4 * (int64_t)ix_cap, cdiv(sp->n_po, IX_BT * 16)));
            MR_TRY(rent.alloc(ctx, (size_t)sp->n_po));
            MR_TRY(rtab.alloc(ctx, (size_t)nshare * (nrange + 1)));
            hipLaunchKernelGGL(k_ix_rpart, dim3(nshare), dim3(IX_BT), 0, st, b.tflag.p, sp->n_po, sp->po_tr.p, sp->po_op.p,
                               sp->po_cnt.p, sp->po_first.p, (int32_t)nrange, rent.p, rtab.p);
        }
        // edges in edge-id order when the table keeps them (large tables) and the counts do not sit
        // in LDS beside the histogram: a segmented sum per id (k_ix_ecount) instead of k_ix_stats'
        // atomic or hash probe per entry; sharded builds then insert each id's count into the hash set
        const char* ebe = getenv("MR_IX_EB");   // (read per call) "0": never
        const bool eb = sp->eb_eid.p && sp->n_ed > 0 && !(ebe && !strcmp(ebe, "0")) &&
                        (!lds_ek || (ebe && !strcmp(ebe, "force")));
        hipLaunchKernelGGL(k_ix_stats, dim3(nrange, nblk), dim3(IX_BT), lds, st, b.tflag.p, sp->n_po, sp->po_tr.p, sp->po_op.p,
                           sp->po_cnt.p, sp->po_first.p, eb ? (int64_t)0 : sp->n_ed, sp->ed_tr.p, sp->ed_key.p, sp->ed_cnt.p,
                           NP, use_lds, b.ocnt.p, b.ofirst.p, b.ocov.p, b.gk.p, b.gc.p, ecap - 1,
                           b.dense ? (const int32_t*)sp->ed_eid.p : nullptr, (int32_t)ecap, lds_ek,
                           (const int4*)rent.p, (const int32_t*)rtab.p, nshare);
        if (eb) {
            const int64_t E = sp->n_edge_keys;
            DBuf<uint64_t> tb;
            DBuf<uint32_t> idc;   // (sharded: the per-id counts before the hash set)
            MR_TRY(tb.alloc(ctx, (size_t)cdiv((int64_t)NT, 64)));
            if (!b.dense) MR_TRY(idc.zero(ctx, (size_t)E));
            hipLaunchKernelGGL(k_tbits, dim3(cdiv((int64_t)NT, 256)), dim3(256), 0, st, b.tflag.p, NT, tb.p);
            hipLaunchKernelGGL(k_ix_ecount, dim3(cdiv(sp->n_ed, 256 * EC_CH)), dim3(256), 0, st, sp->eb_tr.p, sp->eb_cnt.p,
                               sp->eb_eid.p, sp->n_ed, tb.p, b.dense ? b.gc.p : idc.p);
            if (!b.dense)
                hipLaunchKernelGGL(k_ix_edense_hash, dim3(cdiv(E, 256)), dim3(256), 0, st, sp->ekey.p, idc.p, E, b.gk.p,
                                   b.gc.p, ecap - 1);
        }
    }
    if (sp->n_xj)
        hipLaunchKernelGGL(k_ix_cross, dim3(cdiv(sp->n_xj, 256)), dim3(256), 0, st, d_mask, sp->xj_tc.p, sp->xj_tp.p,
                           sp->xj_key.p, sp->n_xj, b.gk.p, b.gc.p, ecap - 1,
                           b.dense ? (const int32_t*)sp->xj_eid.p : nullptr);
    MR_TRY(mr_cross_join_add(ctx, sp, d_mask, X, b.gk.p, b.gc.p, ecap - 1));
    b.small = !sharded && NP <= NS_PMAX;
    if (b.small) {
        // one launch for the node order and P_ss, the trace rows / op lists into upper-bound
        // buffers right behind it; the sizes (N, E, T, nnz) go to d_out
        IxSmall d;
        MR_TRY(mr_ix_small_buffers(ctx, sp, b, g, d_out, &d));
        const NsArgs& a = d.ns;
        hipLaunchKernelGGL(k_nodes_small, dim3(1), dim3(NS_T), 0, st, b.gkp, a.gc, (int64_t)ecap, a.ocnt, a.ofirst, NP,
                           a.node_of_code, a.node_podop, a.len_o, a.nchild, a.ocov, a.cov, a.ss_par, a.ss_off, a.T_dev,
                           a.nnz_dev, a.rs_off, a.out);
        ix_traces_launch(ctx, sp, b, g);
    }
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;
}

static int ix_finish(mr_ctx* ctx, const mr_spans* sp, mr_graph* g, IxBuild& b, const int64_t* h, bool sharded) {
    hipStream_t st = ctx->stream;
    const int32_t NT = sp->n_traces, NP = sp->n_podops;
    if (b.small && h && !h[2]) {
        g->N = (int32_t)h[0];
        g->E = h[1];
        g->T = (int32_t)h[3];
        g->nnz_sr = g->nnz_rs = h[4];
        g->cov_ready = true;
        return MR_OK;
    }
    // the general node order (sharded graphs; more call edges than the one-block path holds)
    MR_TRY(mr_build_nodes(ctx, g, NP, b.ocnt.p, b.ofirst.p, b.ocov.p, sp->row_bits, b.gkp, b.gc.p, b.ecap, b.node_of_code,
                       nullptr, sharded));
    int64_t hh[2] = {0, 0};   // T, nnz (their scans ran before build_nodes' syncs)
    MR_TRY_HIP(ctx, hipMemcpyAsync(&hh[0], b.tpos.p + NT, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipMemcpyAsync(&hh[1], b.zoff.p + NT, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    const int32_t T = (int32_t)hh[0];
    const int64_t nnz = hh[1];
    MR_TRY(g->trace_code.alloc(ctx, T));
    MR_TRY(g->len_t.alloc(ctx, T));
    MR_TRY(g->rs_ops.alloc(ctx, nnz));
    MR_TRY(g->rs_off.alloc(ctx, T + 1));
    ix_traces_launch(ctx, sp, b, g);
    mr_set_last(ctx, g->rs_off.p, T, nnz);
    MR_TRY_HIP(ctx, hipGetLastError());
    g->T = T;
    g->nnz_sr = g->nnz_rs = nnz;
    return MR_OK;
}

int mr_graph_build_indexed(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, mr_graph* g, bool sharded) {
    IxBuild b;
    DBuf<int64_t> dout;
    MR_TRY(dout.alloc(ctx, 8));
    MR_TRY(ix_launch(ctx, sp, d_mask, g, b, dout.p, sharded));
    int64_t h[5] = {0, 0, 0, 0, 0};   // N, E, overflow, T, nnz
    if (b.small) MR_TRY(mr_read_words(ctx, dout.p, 5, h));
    return ix_finish(ctx, sp, g, b, b.small ? h : nullptr, sharded);
}

int mr_ix_launch(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, mr_graph* g, IxBuild& b, int64_t* d_out) {
    return ix_launch(ctx, sp, d_mask, g, b, d_out, false);
}
int mr_ix_finish(mr_ctx* ctx, const mr_spans* sp, mr_graph* g, IxBuild& b, const int64_t* h) {
    MR_TRY(ix_finish(ctx, sp, g, b, h, false));
    return mr_graph_post_build(ctx, g);
}
int mr_ix_finish_unprepared(mr_ctx* ctx, const mr_spans* sp, mr_graph* g, IxBuild& b, const int64_t* h) {
    MR_TRY(ix_finish(ctx, sp, g, b, h, false));
    g->rs_is_sr = true;   // (mr_graph_post_build's fields)
    g->pr_identity = true;
    g->n_pr = g->T;
    return MR_OK;
}
