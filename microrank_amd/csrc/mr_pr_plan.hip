// The first step of a ranking attempt after the set-up (pagerank_attempt, mr_pagerank.hip): the launch
// plan of the fused iteration -- block size, su mode, pf, float su (fx_plan), the LDS image and the
// resident blocks that follow from it -- and the cut of every fused graph's wave tiles into k_tr_a's
// blocks and per-wave runs (cut_blocks: batch_blocks, tr_split, the k_tr_cut kernels).
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <queue>
#include <tuple>

#include "mr_pr_iter.h"
#include "mr_sort.h"

namespace {

// ---------------------------------------------------------------- k_tr_a's per-wave cuts (tr_split, cut_blocks)
// k_tr_a's per-wave runs of tiles of about equal cost (chunks + 2 per tile: a tile's q / r words
// weigh about two chunks), in one block on the device (no host round trip): cut[i] = first tile
// whose cost prefix reaches total * i / nw.  A block (NW waves) must stay within 1023 tiles (65472
// traces: the fixed-point budget); a cost cut that breaks it falls back to equal tile counts (the
// host sizes the grid so those fit).  scale = {2^SC, 2^-SC}: SC = 64 - bits(most traces of a block)
// (the finest scale whose row entries stay below 2^64), or scfix > 0: a scale that does not depend
// on the cut -- window graphs (layout order) take 64 - bits(min(T, 65472)), so a trace's X, hence
// every exact limb sum, is the same however a batch's group cuts the graph into blocks, and a window
// ranks bitwise alike in any batch or group.
constexpr int TC_T = 1024, TC_MAX = 16384;
__device__ __forceinline__ void tr_cut_body(const int32_t* coff, int32_t W, int32_t nw, int32_t NW, int32_t* cut,
                                            double* scale, double tw, int scfix) {
    __shared__ int32_t lc[TC_MAX + 1];
    __shared__ int32_t mx;
    if (threadIdx.x == 0) mx = 0;
    const double total = W ? (double)coff[W] + tw * (double)W : 0.0;
    for (int32_t i = threadIdx.x; i <= nw; i += TC_T) {
        const double target = total * (double)i / (double)nw;
        int32_t lo = 0, hi = W;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if ((double)coff[mid] + tw * (double)mid < target) lo = mid + 1;
            else hi = mid;
        }
        lc[i] = i == nw ? W : lo;
    }
    __syncthreads();
    const int32_t nb = nw / NW;
    for (int32_t b = threadIdx.x; b < nb; b += TC_T) atomicMax(&mx, lc[(b + 1) * NW] - lc[b * NW]);
    __syncthreads();
    if (mx > 1023) {   // (uniform: read after the barrier)
        __syncthreads();
        if (threadIdx.x == 0) mx = 0;
        for (int32_t i = threadIdx.x; i <= nw; i += TC_T) lc[i] = (int32_t)((int64_t)W * i / nw);
        __syncthreads();
        for (int32_t b = threadIdx.x; b < nb; b += TC_T) atomicMax(&mx, lc[(b + 1) * NW] - lc[b * NW]);
        __syncthreads();
    }
    for (int32_t i = threadIdx.x; i <= nw; i += TC_T) cut[i] = lc[i];
    if (threadIdx.x == 0) {
        const int sc = scfix > 0 ? scfix : __clzll((unsigned long long)max(mx, 1) * WAVE);   // 64 - bits(traces)
        scale[0] = __longlong_as_double((long long)(1023 + sc) << 52);
        scale[1] = __longlong_as_double((long long)(1023 - sc) << 52);
    }
}
__global__ void __launch_bounds__(TC_T) k_tr_cut(const int32_t* coff, int32_t W, int32_t nw, int32_t NW, int32_t* cut,
                                                 double* scale, double tw, int scfix) {
    tr_cut_body(coff, W, nw, NW, cut, scale, tw, scfix);
}
// the cuts of a batch's graphs in one launch (block g: graph g)
struct CutArg {
    const int32_t* coff;
    int32_t* cut;
    double* scale;
    int32_t W, nw, NW;
    float tw;   // a tile's fixed cost in chunks
    int32_t scfix;   // > 0: the graph's cut-independent scale
};
constexpr int TC_BATCH = 64;
struct CutBatch {
    CutArg a[TC_BATCH];
};
__global__ void __launch_bounds__(TC_T) k_tr_cut_b(CutBatch b) {
    const CutArg& x = b.a[blockIdx.x];
    tr_cut_body(x.coff, x.W, x.nw, x.NW, x.cut, x.scale, (double)x.tw, x.scfix);
}

}  // namespace

// ---------------------------------------------------------------- the plan
// allow_pf false: k_fx_b every iteration, as under MR_TR_PF=0 (a call that reads the ring between launches)
FxPlan fx_plan(mr_graph* const* gs, int ng, bool fp32, bool sharded, bool allow_pf) {
    FxPlan P;
    int32_t nmax = 0;
    int64_t tmax = 0;
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused) {
            nmax = std::max(nmax, kern_n(gs[i]));
            tmax = std::max<int64_t>(tmax, gs[i]->T);
        }
    // 1024-thread blocks when the largest graph has a wave tile for every wave of the chip (and
    // always for graphs with register-accumulated hot ops: only that variant carries them)
    P.NT = cdiv(tmax, WAVE) >= (int64_t)num_cus() * 16 ? 1024 : 512;
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused && gs[i]->nhr) P.NT = 1024;
    bool relabeled = false;
    for (int i = 0; i < ng; ++i) relabeled = relabeled || (gs[i]->fused && gs[i]->relabeled);
    P.sul = TrLds(nmax, WV_SU_ALL).su_lds;
    P.mode = P.sul ? WV_SU_ALL : relabeled ? WV_SU_HOT : WV_SU_GLOBAL;
    if (P.mode == WV_SU_HOT)   // every graph of the launch must be relabelled (hot ops = low labels)
        for (int i = 0; i < ng; ++i)
            if (gs[i]->fused && !gs[i]->relabeled) P.mode = WV_SU_GLOBAL;
    if (P.mode == WV_SU_HOT && TrLds(nmax, WV_SU_HOT).n_hot < 64) P.mode = WV_SU_GLOBAL;
    // window batches: the next launch's blocks finish an iteration (k_tr_a pf), no k_fx_b between
    // launches -- every graph fused and plain (no multiplicities, cold sums, merged runs, hot
    // ops or relabelling), N <= PF_NMAX (three N-word LDS arrays, four blocks per CU).
    // MR_TR_PF=0 (read per call; A/B and tests): k_fx_b every iteration
    P.pf = allow_pf && knob_on("MR_TR_PF") && !sharded && ng >= 2 && P.NT == 512 && P.mode == WV_SU_ALL;
    for (int i = 0; i < ng && P.pf; ++i) {
        const mr_graph* g = gs[i];
        P.pf = g->fused && !g->wide && !g->relabeled && !g->nhr && !g->mw_tp.p && kern_n(g) <= PF_NMAX &&
               !(g->lo && g->lo_merged == 1);
    }
    // fp32 wide graphs: su as floats in k_tr_a's LDS, the freed half holding the next ~10k
    // ("warm") labels' su, so their cold entries read LDS instead of L2 (k_tr_a EXT & TR_X_W32);
    // every fused graph of the launch wide and plain (no multiplicities)
    P.w32 = fp32 && P.mode == WV_SU_ALL && !P.pf;
    bool anyf = false;
    for (int i = 0; i < ng && P.w32; ++i)
        if (gs[i]->fused) {
            anyf = true;
            P.w32 = gs[i]->wide && !gs[i]->mw_tp.p && !gs[i]->trun.p;
        }
    P.w32 = P.w32 && anyf;
    return P;
}
int32_t plan_n_hot(int32_t N, const FxPlan& P) {
    return P.mode == WV_SU_HOT ? TrLds(N, WV_SU_HOT).n_hot : 0;
}
size_t plan_lds(int32_t N, const FxPlan& P) { return TrLds(N, P.mode, P.pf, P.w32).total; }
bool tr_su_fits(int32_t N) { return TrLds(N, WV_SU_ALL).su_lds; }
bool tr_hot_fits(int32_t N) { return TrLds(N, WV_SU_ALL).hot_ok; }

// resident blocks of the plan's kernel on the chip (occupancy by LDS image and VGPRs)
static int64_t plan_resident(int32_t N, const FxPlan& P) {
    const size_t lds = plan_lds(N, P);
    // (cached per (mode, block size, LDS bytes): a window group asks for each of its 256 graphs)
    static std::mutex mu;
    static std::map<std::tuple<int, int, size_t>, int> cache;
    const auto key = std::make_tuple(P.mode, P.NT, lds);
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = cache.find(key);
        if (it != cache.end()) return (int64_t)num_cus() * it->second;
    }
    const TrA kfn = tr_kernel(false, P.mode, P.NT, 0);
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)kfn, P.NT, lds) != hipSuccess || n < 1)
        n = std::max<int>(1, (int)(WV_LDS_MAX / std::max<size_t>(lds, 1)));
    std::lock_guard<std::mutex> lk(mu);
    cache[key] = n;
    return (int64_t)num_cus() * n;
}

// k_tr_a: blocks of one graph and the cut of its tiles into contiguous per-wave runs of about
// equal cost (chunks + 2 per tile: a tile's q/r words weigh about two chunks).  Cached per
// graph for the wave count; at most 1023 tiles (65472 traces) per block.
// wsum: wave tiles of all fused graphs of the launch.  A graph of a batch gets its share of the
// resident blocks in proportion to its tiles: a small graph of a batch then runs a few blocks with
// several tiles per wave instead of one block per tile set -- the per-block fixed cost (LDS image,
// the N-word partial row written here and re-read by k_fx_b) falls with the block count while the
// batch still fills the chip.
// a tile's fixed cost in chunks for the per-wave cut: its q / r words and r' (about two chunks),
// plus the hot-op accumulators and mask sum on hot-op layouts (3: with 2 the waves of short hot
// tiles became a tail, C4 188 us per iteration)
static double tr_tile_weight(const mr_graph* g) { return g->nhr ? 3.0 : 2.0; }
// window graphs (layout order, ranked in batches whose groups cut them differently): the fixed-point
// scale from the graph's trace count -- a bound for any block of any cut -- instead of the cut's
// largest block (tr_cut_body); 0 for other graphs (the finest scale of their cut)
int32_t tr_scfix(const mr_graph* g) {
    return g->lo ? 64 - bits_for((uint64_t)std::min<int64_t>(std::max<int32_t>(g->T, 1), 1023 * WAVE)) : 0;
}
static int tr_split(mr_ctx* ctx, mr_graph* g, const FxPlan& P, int64_t wsum, int64_t* nfa,
                    std::vector<CutArg>* defer = nullptr, int64_t force_nb = 0) {
    const int64_t W = g->n_wt, NW = P.NT / WAVE;
    const int64_t resident = plan_resident(kern_n(g), P);
    int64_t nb = std::max<int64_t>({std::min<int64_t>(resident, cdiv(W, NW)), cdiv(W, 1023), 1});
    if (const char* fe = getenv("MR_TR_BLOCKS"))   // (A/B knob, read per call) blocks of a lone graph
        if (force_nb <= 0 && wsum <= W && atoi(fe) > 0) force_nb = atoi(fe);
    if (force_nb > 0) {   // (at most 1023 wave tiles per block still)
        nb = std::max<int64_t>(force_nb, cdiv(W, 1023));
    } else {
        if (wsum > W) {
            const int64_t share = (int64_t)std::ceil((double)resident * (double)W / (double)wsum);
            nb = std::min(nb, share);
        }
        // at least two tiles per wave: a launch of few tiles (one window's graphs) otherwise runs a
        // block per 8 tiles, each paying its LDS image and an N-word partial row for them (C2 single
        // window: 365 blocks of one tile per wave 0.85 ms, ~180 blocks 0.78 ms; batches and whole
        // graphs run many tiles per wave and do not reach the cap)
        nb = std::max<int64_t>({std::min<int64_t>(nb, cdiv(W, 2 * NW)), cdiv(W, 1023), 1});
    }
    // on the device (k_tr_cut: no host round trip) unless a block's traces must be weighed by
    // their kinds' multiplicities (kind-compressed graphs) or the cut table exceeds its LDS
    if (g->tile_mult_h.empty() && nb * NW <= TC_MAX) {
        const int64_t nw = nb * NW;
        if (!(g->wtile.p && g->wtile_nw == nw && g->wtile_msum < 0)) {
            MR_TRY(g->wtile.alloc(ctx, (size_t)nw + 1));
            MR_TRY(g->dscale.alloc(ctx, 2));
            if (defer) {   // launched with the batch's other cuts (k_tr_cut_b)
                defer->push_back(CutArg{g->coff.p, g->wtile.p, g->dscale.p, (int32_t)W, (int32_t)nw, (int32_t)NW,
                                        (float)tr_tile_weight(g), tr_scfix(g)});
            } else {
                hipLaunchKernelGGL(k_tr_cut, dim3(1), dim3(TC_T), 0, ctx->stream, g->coff.p, (int32_t)W, (int32_t)nw,
                                   (int32_t)NW, g->wtile.p, g->dscale.p, tr_tile_weight(g), tr_scfix(g));
                MR_TRY_HIP(ctx, hipGetLastError());
            }
            g->wtile_nw = (int32_t)nw;
            g->wtile_msum = -1;   // the scale is on the device
        }
        *nfa = nb;
        return MR_OK;
    }
    if (g->coff_h.size() != (size_t)W + 1) {
        g->coff_h.assign((size_t)W + 1, 0);
        MR_TRY(g->coff.download(ctx, g->coff_h.data(), (size_t)W + 1));
        MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const std::vector<int32_t>& co = g->coff_h;
    for (;;) {
        const int64_t nw = nb * NW;
        if (g->wtile.p && g->wtile_nw == nw && g->wtile_msum >= 0) break;
        std::vector<int32_t> cut((size_t)nw + 1);
        const double tw = tr_tile_weight(g);
        const double total = W ? (double)co[(size_t)W] + tw * (double)W : 0.0;
        int64_t k = 0;
        for (int64_t i = 0; i <= nw; ++i) {   // first tile whose cost prefix reaches the target
            const double target = total * (double)i / (double)nw;
            while (k < W && (double)co[(size_t)k] + tw * (double)k < target) ++k;
            cut[(size_t)i] = (int32_t)k;
        }
        cut[(size_t)nw] = (int32_t)W;
        int32_t tpb = 0;
        int64_t msum = 0;   // traces a block stands for (kind-compressed graphs: with multiplicity)
        for (int64_t b = 0; b < nb; ++b) {
            const int32_t k0 = cut[(size_t)(b * NW)], k1 = cut[(size_t)((b + 1) * NW)];
            tpb = std::max(tpb, k1 - k0);
            int64_t m = (int64_t)(k1 - k0) * WAVE;
            if (!g->tile_mult_h.empty()) {
                m = 0;
                for (int32_t k = k0; k < k1; ++k) m += g->tile_mult_h[(size_t)k];
            }
            msum = std::max(msum, m);
        }
        if (tpb > 1023) {
            nb += resident;
            continue;
        }
        g->wtile_msum = msum;
        MR_TRY(g->wtile.upload(ctx, cut.data(), cut.size()));
        MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the host vector leaves scope)
        g->wtile_nw = (int32_t)nw;
        g->wtile_tpb = tpb;
        break;
    }
    *nfa = nb;
    return MR_OK;
}

// k_tr_a blocks of every graph of a batch launch: ONE resident set of blocks, split by the graphs'
// wave tiles so that the largest per-block share is as small as it can be -- each graph first gets
// floor(resident x its tiles / all tiles) blocks (at least one, at least its 1023-tile cap, at most
// one per two tiles per wave), then the remaining blocks go one at a time to the graph whose blocks
// carry the most tiles.  (Rounding each graph's share UP put 1152 blocks on the 1024 resident slots
// of a C2 group -- 128 windows' 13k- and 187k-trace graphs, 7.5 and 0.5 blocks of share each: a
// second round of blocks behind the first.)  Empty: the single-graph rule of tr_split.
#ifndef MR_TR_TPW
#define MR_TR_TPW 2   // batch launches: at least this many wave tiles per wave of a graph's blocks
#endif
static std::vector<int64_t> batch_blocks(mr_graph* const* gs, int ng, const FxPlan& P, int64_t wsum) {
    std::vector<int64_t> nb;
    int nf = 0;
    for (int i = 0; i < ng; ++i) nf += gs[i]->fused ? 1 : 0;
    if (nf < 2 || wsum <= 0) return nb;
    int64_t R = INT64_MAX;
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused) R = std::min(R, plan_resident(kern_n(gs[i]), P));
    // (two or three blocks per resident slot measured 2-3 % faster per iteration inside the pipeline
    // and within the wall-time spread, profiles/r06/r06i_oversub_ab.txt: one set kept)
    const int64_t NW = P.NT / WAVE;
    nb.assign((size_t)ng, 0);
    std::vector<int64_t> cap((size_t)ng, 0);
    int64_t used = 0;
    for (int i = 0; i < ng; ++i) {
        if (!gs[i]->fused) continue;
        const int64_t W = gs[i]->n_wt, lo = std::max<int64_t>(cdiv(W, 1023), 1);
        cap[(size_t)i] = std::max<int64_t>(lo, cdiv(W, (int64_t)MR_TR_TPW * NW));
        nb[(size_t)i] = std::min(cap[(size_t)i], std::max(lo, (int64_t)((double)R * (double)W / (double)wsum)));
        used += nb[(size_t)i];
    }
    std::priority_queue<std::pair<double, int>> q;   // (tiles per block, graph)
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused && nb[(size_t)i] < cap[(size_t)i])
            q.push({(double)gs[i]->n_wt / (double)nb[(size_t)i], i});
    while (used < R && !q.empty()) {
        const int i = q.top().second;
        q.pop();
        ++nb[(size_t)i];
        ++used;
        if (nb[(size_t)i] < cap[(size_t)i]) q.push({(double)gs[i]->n_wt / (double)nb[(size_t)i], i});
    }
    return nb;
}

// The k_tr_a blocks of every graph (nfa[i]; 0 for a graph off the fused path): ONE tr_split per fused
// graph, its partial rows allocated, and the launch's per-wave cuts in batches (k_tr_cut_b).
int cut_blocks(mr_ctx* ctx, mr_graph* const* gs, int ng, const FxPlan& plan, HostMarks& hm,
               std::vector<int64_t>& nfa) {
    int64_t wsum = 0;   // wave tiles of the launch's fused graphs (k_tr_a's block budget)
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused) wsum += gs[i]->n_wt;
    std::vector<CutArg> cuts;   // the graphs' per-wave cuts, launched together
    // a batch's forced block counts, each replaced by its graph's blocks as tr_split returns them
    // (empty: the single-graph rule, force 0)
    nfa = batch_blocks(gs, ng, plan, wsum);
    if (nfa.empty()) nfa.assign((size_t)ng, 0);
    for (int i = 0; i < ng; ++i) {
        mr_graph* g = gs[i];
        if (!g->fused) continue;
        int64_t& nb = nfa[(size_t)i];   // the plan's blocks: partial rows and (k_tr_a) the per-wave cut
        MR_TRY(tr_split(ctx, g, plan, wsum, &nb, &cuts, nb));
        // (pf: rows and call-graph terms double-buffered, iteration it & 1)
        MR_TRY(g->fx_part.alloc(ctx, (size_t)(plan.pf ? 2 : 1) * std::max<int64_t>(nb, 1) * (size_t)kern_n(g)));
        if (plan.pf) MR_TRY(g->fx_ssv.alloc(ctx, 2 * (size_t)g->N));
    }
    hm.mark("blocks");
    for (size_t c0 = 0; c0 < cuts.size(); c0 += TC_BATCH) {
        CutBatch cb;
        const size_t n = std::min<size_t>(TC_BATCH, cuts.size() - c0);
        for (size_t j = 0; j < n; ++j) cb.a[j] = cuts[c0 + j];
        hipLaunchKernelGGL(k_tr_cut_b, dim3((unsigned)n), dim3(TC_T), 0, ctx->stream, cb);
        MR_TRY_HIP(ctx, hipGetLastError());
    }
    return MR_OK;
}
