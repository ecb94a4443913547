// The second step of a ranking attempt (pagerank_attempt, mr_pagerank.hip): the launch described --
// every graph's device descriptor (GDev, mr_iter_dev.h) filled in three parts, gdev_pointers,
// gdev_scales and gdev_launch; then what the launch as a whole takes from them (finalise_launch: the
// k_tr_a variant, the one-CU rule, pf, k_fx_b's block size) and what it needs beside them
// (prepare_exchange: the side stream, a sharded graph's peer exchange).
#include <cmath>
#include <cstdlib>

#include "mr_pr_iter.h"
#include "mr_sort.h"

// ops per k_fx_b block: a lane reads op (lane % ops) of every (64/ops)-th row of its wave's share,
// so a row read stays one 128-B line per op group while small graphs still spread over many CUs
// A batch of many small graphs (C2 / C3 window groups: thousands of 16-op blocks, several rounds
// of the chip) takes 64 ops per block instead: lane = op, one row group per wave -- the same
// integer limb sums and call-graph terms, so bitwise the same results.  MR_FB_OPS: force 16 / 32 /
// 64 (read per call: tests)
static int fb_ops(int32_t N, bool many) {
    const char* e = getenv("MR_FB_OPS");
    const int force = e ? atoi(e) : 0;
    if (force == 16 || force == 32 || force == 64) return force;
    // (> 8192 ops: 64 measured ahead of 32 -- C4 140.0 -> 137.8 us per iteration, its rank-0-of-8
    // share 43.6 -> 41.5 us, C5 2.97 -> 2.94 ms; profiles/r05/r05q_fb_ops64_ab.txt)
    return N <= 8192 ? (many ? 64 : 16) : 64;
}

// algorithmic bytes of one iteration of one graph: op ids once, offsets, the
// r/v/len_t streams, call edges and three N-vectors; o = 4-byte offsets below 2^31 nonzeros
static double iter_bytes(const mr_graph* g, bool fp32) {
    const double w = fp32 ? 4.0 : 8.0, o = g->nnz_sr < (1ll << 31) ? 4.0 : 8.0;
    return 4.0 * (double)g->nnz_sr + o * ((double)g->T + 1) + 4.0 * w * (double)g->T + (8.0 + w) * (double)g->E +
           3.0 * w * (double)g->N;
}

// A graph's descriptor, part 1: its arrays and sizes, field for field
void gdev_pointers(GDev& v, const mr_ctx* ctx, const mr_graph* g, bool fp32, double alpha, const FxPlan& plan) {
    v.rs_off = g->rs_off.p;
    v.rs_ops = g->rs_ops.p;
    v.rs16 = g->rs16.p;
    v.rsw = g->relabeled ? g->rsp.p : g->rs16.p;
    v.perm = g->relabeled ? g->perm.p : nullptr;
    v.n_hot = plan_n_hot(kern_n(g), plan);
    v.tids = g->tids.p;
    v.coff = g->coff.p;
    v.wtile = g->wtile.p;
    v.c_tp = g->c_tp.p;
    v.w_tp = g->w_tp.p;
    v.mw_tp = g->mw_tp.p;
    v.hmask = g->nhr ? g->hmask.p : nullptr;
    v.trun = g->lo && g->lo_merged == 1 ? g->trun.p : nullptr;   // (set at prepare: the ids' rotation follows it)
    v.ctids = g->wide ? g->ctids.p : nullptr;
    v.ccoff = g->wide ? g->ccoff.p : nullptr;
    v.nhr = g->fused ? g->nhr : 0;
    for (int h = 0; h < 8; ++h) v.hop[h] = g->hop[h];
    v.c_t = g->c_t.p;
    v.w_t = g->w_t.p;
    v.u_o = g->u_o.p;
    v.pw = g->pw.p;
    v.ltr = g->tl_ltr.p;
    v.pr_beg = g->pr_beg.p;
    v.tile_pr0 = g->tile_pr0.p;
    v.lp = g->lp.p;
    v.tile_lp0 = g->tile_lp0.p;
    v.op_pr_off = g->op_pr_off.p;
    v.op_pr = g->op_pr.p;
    v.ss_off = g->ss_off.p;
    v.ss_par = g->ss_par.p;
    for (int j = 0; j < 2; ++j) {
        v.q[j] = fp32 ? (void*)g->q32[j].p : (void*)g->q64[j].p;
        v.sub[j] = g->sub[j].p;
        v.suf[j] = g->suf[j].p;
        v.spb[j] = g->spb[j].p;
    }
    v.part = g->part.p;
    v.mslot = g->mslot.p;
    v.sn = g->sn.p;
    v.weight = g->weight.p;
    v.scal = g->scal.p;
    v.flag = g->flag.p;
    v.fx_part = (unsigned long long*)g->fx_part.p;
    v.fx_ssv = g->fx_ssv.p;
    v.fx_limb = (unsigned long long*)g->fx_limb.p;
    v.op_sum = g->op_sum.p;
    v.rank = ctx->rank;
    v.nranks = ctx->nranks;
    v.alpha = alpha;
    v.T = g->T;
    v.N = g->N;
    v.NA = kern_n(g);
    v.cold_rw = g->cold_rw;
    v.ns_warm = plan.w32 ? v.NA + std::min(TrLds(v.NA, WV_SU_ALL, false, true).n_warm, g->N - v.NA) : v.NA;
    v.su32 = fp32 && g->wide;
    v.cold_acc = g->wide ? g->cold_acc.p : nullptr;
    v.cold_part = (const unsigned long long*)g->cold_part.p;
    v.cold_rowbase = g->cold_rowbase.p;
}

// Part 2: the fixed-point scales of the partial rows (fx_*), of a wide graph's cold rows (cx_*), and
// the scale a device cut left on the device (dscale)
void gdev_scales(GDev& v, const mr_graph* g, bool sharded, uint64_t cold_span_all) {
    // a row entry stays below 2^64 (traces per block < 2^(64-sc)).  Shards of one graph hold
    // different trace counts and their limbs are summed, so they share one scale, 2^48 (<= 65535
    // traces per block: wv_blocks / fx_blocks); window graphs take their cut-independent scale
    // (tr_scfix); a graph cut on the device carries its scale there (dscale)
    const int64_t tpb = g->fused ? g->wtile_msum : 0;
    const int sc = sharded ? 48 : tr_scfix(g) > 0 ? tr_scfix(g) : 64 - bits_for((uint64_t)std::max<int64_t>(tpb, 1));
    int sf = sc, sx = sc;   // the rows' and the cold rows' scales (2^sf, 2^sx)
    if (g->wide) {
        // cold rows: at most cold_span adds per op and row; a sharded graph's ranks sum their
        // limbs per op, and an op hot on one rank may be cold on another: one scale for both
        // (the smaller), agreed over the ranks (cold_span_all)
        sx = 64 - bits_for(sharded ? cold_span_all : g->cold_span);
        if (sharded) sf = sx = std::min(sc, sx);
    }
    v.fx_scale = std::ldexp(1.0, sf);
    v.fx_iscale = std::ldexp(1.0, -sf);
    v.cx_scale = std::ldexp(1.0, sx);
    v.cx_iscale = std::ldexp(1.0, -sx);
    // the graph's scale on the device (k_tr_cut) unless the ranks share the fixed one
    v.dscale = (!sharded && g->fused && g->wtile_msum < 0) ? g->dscale.p : nullptr;
}

// Part 3: the graph's blocks in each of the iteration's launches (nfa: its k_tr_a blocks, cut_blocks)
// and the form its iterations take; the launch's totals grow by them
void gdev_launch(GDev& v, const mr_graph* g, int64_t nfa, bool fp32, bool sharded, const FxPlan& plan,
                 const TrKnobs& kn, bool fb_many, Launch& L) {
    // a shard without traces still runs one (empty) block: it clears the maxima slot and
    // writes a zero partial row, and the collectives after the launch need every rank
    nfa = g->fused ? std::max<int64_t>(nfa, sharded ? 1 : 0) : 0;
    v.blk0f = L.blocks_fa;
    v.n_fa = (int32_t)nfa;
    L.blocks_fa += v.n_fa;
    v.blk0fb = L.blocks_fb;
    v.fb_ops = fb_ops(g->N, fb_many);
    // the last k_tr_a block finishes small graphs itself (window batches: one launch per
    // iteration); its sc1 row reads stay short: at most LASTFIN_WORDS row words
    // (ops <= threads: the finishing block takes every op in one round -- C3's 500-op windows;
    // C2's 1000-op windows measured -1.5 % with it, C3 +6.5 % windows/s, -7 % single window)
    v.lastfin = kn.lastfin && plan.NT == 512 && !sharded && g->fused && !g->wide && !g->relabeled &&
                plan.mode == WV_SU_ALL && nfa >= 1 && g->N <= plan.NT && nfa * (int64_t)g->N <= LASTFIN_WORDS;
    v.n_fb = g->fused && !v.lastfin ? cdiv(g->N, v.fb_ops) : 0;
    // the call-graph terms in k_tr_a (large graphs: k_fx_b's chains of dependent loads leave its
    // critical path; not for wide graphs: k_fx_b's columns past NA).  Last-block graphs: every
    // block writes its share write-through and the last block reads the terms with one load per
    // op instead of the ss_off -> ss_par -> pw / s_k chain (MR_TR_LFSSV=0: the chain; read per call)
    v.ssv_pre = kn.ssv && nfa >= 1 && !g->wide && ((v.n_fb > 0 && g->N >= 2048) || (v.lastfin && kn.lfssv));
    v.pf = plan.pf && !v.lastfin && nfa <= PF_ROWS;
    v.pf_stride = nfa * (int64_t)kern_n(g);
    if (v.pf) v.ssv_pre = 1;   // (the next launch's prologue reads the terms: one load per op)
    v.row_wt = kn.row_wt && g->N >= 2048;
    L.blocks_fb += v.n_fb;
    v.blk0 = L.blocks_a;
    v.blk0b = L.blocks_b;
    v.blk0r = L.blocks_r;
    L.blocks_r += cdiv(g->N, RESID_OPS);
    L.bytes += iter_bytes(g, fp32);
    if (g->fused) {   // no tile-path blocks (n_tb = n_tiles = n_ob = 0)
        L.lds_f = std::max(L.lds_f, plan_lds(kern_n(g), plan));
        return;
    }
    v.n_tb = std::max(cdiv(g->T, TB), sharded ? 1 : 0);   // (empty shard: see nfa)
    v.n_tiles = g->n_tiles;
    v.tshift = g->tshift;
    v.lds_su = g->N <= LDS_NODES;
    L.blocks_a += v.n_tb + v.n_tiles;
    v.n_ob = cdiv(g->N, TB / WAVE);
    L.blocks_b += v.n_ob;
    if (v.lds_su) L.lds = std::max(L.lds, ((size_t)g->N + VCAP) * sizeof(double));
    L.lds = std::max(L.lds, ((size_t)1 << g->tshift) * (fp32 ? sizeof(float) : sizeof(double)));
}

// The launch's variant, from its graphs' descriptors: the one-CU rule, the k_tr_a kernel, whether every
// graph finishes in-kernel (launch_pf), k_fx_b's block size.  Rejects the two batches no variant runs.
int finalise_launch(mr_ctx* ctx, mr_graph* const* gs, int ng, bool fp32, bool sharded, const FxPlan& plan,
                    const TrKnobs& kn, std::vector<GDev>& hv, Launch& L) {
    L.split_fa = ng == 2 ? hv[1].blk0f : 0;
    L.split_fb = ng == 2 ? hv[1].blk0fb : 0;
    // last-block graphs: a launch that fits one block per CU runs so (LDS past half a CU), and its
    // finishing blocks skip the acquire (tr_last_finish); else they take it
    bool any_lf = false;
    for (int i = 0; i < ng; ++i) any_lf = any_lf || hv[(size_t)i].lastfin;
    const bool one_cu = LF_ONE_CU_LDS > 0 && any_lf && L.blocks_fa <= num_cus() && LF_ONE_CU_LDS <= WV_LDS_MAX;
    if (one_cu) L.lds_f = std::max(L.lds_f, LF_ONE_CU_LDS);
    for (int i = 0; i < ng; ++i) hv[(size_t)i].lf_acq = one_cu ? 0 : 1;
    for (int i = 0; i < ng; ++i)   // hot-op layouts need every op's su in LDS (a batch with a much wider graph)
        if (gs[i]->fused && gs[i]->nhr && plan.mode != WV_SU_ALL)
            return mr_fail(ctx, MR_ERR_ARG, "pagerank batch: a hot-op layout (T >= MR_TR_HOT_MIN) with a graph of > %d ops",
                           (int)WIDE_NA);
    int any_ext = 0;   // what some fused graph of the launch carries (TR_X_*), then the variant that walks them all
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused)
            any_ext |= (hv[(size_t)i].mw_tp ? TR_X_KINDS : 0) | (hv[(size_t)i].cold_acc ? TR_X_COLD : 0) |
                       (hv[(size_t)i].trun ? TR_X_RUNS : 0);
    const int ext = tr_launch_ext(any_ext, plan.w32);
    for (int i = 0; i < ng; ++i)   // the wide variant carries HOT_MAX_WIDE hot accumulators
        if ((ext & TR_X_COLD) && gs[i]->fused && gs[i]->nhr > HOT_MAX_WIDE)
            return mr_fail(ctx, MR_ERR_ARG, "pagerank batch: a hot-op layout of %d ops beside a wide graph", gs[i]->nhr);
    L.launch_pf = plan.pf;
    for (int i = 0; i < ng; ++i) L.launch_pf = L.launch_pf && (hv[(size_t)i].lastfin || hv[(size_t)i].pf);
    L.launch_pf = L.launch_pf && ext == 0;
    if (!L.launch_pf)
        for (int i = 0; i < ng; ++i) {
            if (hv[(size_t)i].pf) hv[(size_t)i].ssv_pre = kn.ssv && !gs[i]->wide && gs[i]->N >= 2048;
            hv[(size_t)i].pf = 0;
        }
    L.tr_a = tr_kernel(fp32, plan.mode, plan.NT, ext);
    if (!L.tr_a) return mr_fail(ctx, MR_ERR_STATE, "pagerank: no k_tr_a variant %d is built", ext);
    // a wide graph beside a narrow one whose su does not fit in LDS: the launch leaves WV_SU_ALL, and
    // the kernels of the other modes have no short-tile walk (tr_kernel: no EXT variant), so none of
    // the wide graph's tiles gathers its own cold su -- the general walk reads cold_acc for every
    // tile, and k_cold_trace must then have summed every tile, not only the listed ones
    L.cold_all = (ext & TR_X_COLD) && plan.mode != WV_SU_ALL;
    // a sharded graph with no collective backend is one whole shard: the split launches around the
    // (no-op) all-reduces would compute the same integers / sums in two halves
    L.coll = sharded && mr_coll_ready(ctx);
    for (int i = 0; i < ng; ++i) L.any_wide = L.any_wide || gs[i]->wide;
    // k_fx_b's block size: 4 waves when no graph of the launch has many partial rows
    L.fb_small = !L.any_wide;
    // (a large graph alone -- C4: 256 rows of 10k ops -- sums faster with 16-wave blocks: 137 -> 134 us)
    for (int i = 0; i < ng; ++i)
        L.fb_small = L.fb_small && hv[(size_t)i].n_fa <= FB_SMALL_ROWS && hv[(size_t)i].N <= 4096;
    return MR_OK;
}

// What the launches need beside the descriptors: the side stream of a launch with wide graphs, and a
// sharded graph's peer exchange
int prepare_exchange(mr_ctx* ctx, mr_graph* const* gs, int ng, Launch& L) {
    // wide graphs: k_cold_ops (LDS-bound) runs on the side stream beside k_cold_trace (L2-gather
    // bound) and k_tr_a on the main stream; k_fx_b waits for both
    L.sst = ctx->stream;
    if (L.any_wide) {
        if (!ctx->side) {
            MR_TRY_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            for (hipEvent_t& e : ctx->side_ev) MR_TRY_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        L.sst = ctx->side;
    }
    // sharded fused graph on the peer path: the exchange inside k_fx_b (MR_PEER_SPLIT=1: the separate
    // push / reduce launches; relabelled graphs always -- the ranks' op labels differ, so a block's
    // columns on one rank are not the same ops on another)
    if (L.coll && ng == 1 && gs[0]->fused && !gs[0]->wide && !gs[0]->relabeled && mr_peer_ready(ctx) &&
        !getenv("MR_PEER_SPLIT")) {
        const int prc = mr_peer_fx_prepare(ctx, 2 * (int64_t)gs[0]->N + ctx->nranks, L.blocks_fb, &L.px);
        if (prc == MR_OK) {
            L.px_on = true;
            // ranks sharing a device: mode-2 blocks spinning there would hold CUs a peer's 160-KB
            // k_tr_a blocks need -- one waiting block instead (MR_PEER_SPIN=0/1 forces it)
            const char* se = getenv("MR_PEER_SPIN");
            L.px.spin = se ? atoi(se) != 0 : !mr_peer_same_device(ctx);
        } else if (prc != MR_ERR_STATE) {
            return prc;
        }
    }
    return MR_OK;
}
