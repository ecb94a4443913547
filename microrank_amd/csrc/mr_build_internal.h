// Host declarations shared between the graph-build units (mr_graph_build.hip, mr_build_ix.hip,
// mr_build_win.hip, mr_build_lo.hip).  What the rest of the library calls is in mr_internal.h.
#pragma once
#include <algorithm>

#include "mr_build_dev.h"

// ---- mr_graph_build.hip
// the call-edge hash's slots for up to `want` distinct keys over NP pod-ops (a power of two)
inline uint64_t mr_edge_capacity(int64_t want, int32_t NP) {
    const uint64_t w = (uint64_t)std::min<int64_t>(std::max<int64_t>(want, 1), (int64_t)NP * NP + 1);
    uint64_t cap = 1024;
    while (cap < 2 * w) cap <<= 1;
    return cap;
}
// the general node order (any size, sharded graphs): see its definition
int mr_build_nodes(mr_ctx* ctx, mr_graph* g, int32_t NP, const int32_t* ocnt, const int32_t* ofirst, const int32_t* ocov,
                   int row_bits, const uint64_t* gk, const uint32_t* gc, uint64_t ecap, DBuf<int32_t>& node_of_code,
                   PhaseTimer* pt = nullptr, bool sharded = false);
void mr_set_last(mr_ctx* ctx, int64_t* off, int32_t n, int64_t v);   // off[n] = v on the stream
// a sharded build's join across ranks: the other ranks' export records sorted by spanID (keys /
// record index) and the number of cross-rank (child, parent) matches
struct CrossJoin {
    DBuf<uint64_t> rec, key;
    DBuf<uint32_t> val;
    int64_t n = 0;
    int64_t matches = 0;
};
int mr_cross_exchange(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, CrossJoin& X);
int mr_cross_join_add(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, const CrossJoin& X, uint64_t* gk,
                      uint32_t* gc, uint64_t gmask);

// ---- mr_build_ix.hip
int mr_graph_build_indexed(mr_ctx* ctx, const mr_spans* sp, const uint8_t* d_mask, mr_graph* g, bool sharded = false);
// A table within the one-pass limits of a window's two-graph build: dense edge ids, the one-block
// node order, both graphs' histograms in k_ix_stats2_b's LDS.  (mr_lo_fits asks for more.)
inline bool mr_ix2_fits(const mr_spans* sp) {
    return sp->ekey.p && sp->n_podops <= NS_PMAX && 2 * (3 * (int64_t)sp->n_podops + sp->n_edge_keys) <= IX_LDS_WORDS;
}
// The buffers of a graph that ends in the one-block node order, at their upper bounds (the sizes
// come back later): B.node_of_code and G's per-node arrays and P_ss ...
int mr_ix_graph_buffers(mr_ctx* ctx, int32_t NP, IxBuild& B, mr_graph* G);
// ... and with them G's trace rows and op lists, and the three descriptors of the graph over B's
// selection and counters (allocated by the caller): sizes to d_out (N, E, overflow, T, nnz).
struct IxSmall {
    IxSide x;
    NsArgs ns;
    TrOut tr;
};
int mr_ix_small_buffers(mr_ctx* ctx, const mr_spans* sp, IxBuild& B, mr_graph* G, int64_t* d_out, IxSmall* out);

// ---- mr_build_win.hip
// the last two stages of a window batch, general or layout-order: the join pairs across traces
// (bc blocks; none: no launch) and each graph's node order (block 2k + g: window k, graph g)
void mr_ix_cross_nodes_launch(mr_ctx* ctx, int n, int32_t bc, const IxBatch<IxWinCross>& ac, const IxBatch<IxWinNodes>& an);
