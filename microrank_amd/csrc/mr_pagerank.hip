// K2: personalised PageRank of pagerank.trace_pagerank (pagerank.py:15-130) on gfx950.
//
// Sparse, HBM-bound: no MFMA.  Each Jacobi iteration k -> k+1 (T8) is two launches:
//   k_iter_a, two block roles reading only iteration-k state:
//     trace role  r'[t] = d * sum_{o in rs(t)} u_o * s_k[o] + fp32((1-d) v_t)     (pagerank.py:125)
//                 q'[t] = w_t * r'[t]   (the P_sr-weighted value the op side sums next time)
//                 s_k*u staged in LDS; the block's contiguous id range (u16 ids when N <= 65536)
//                 read coalesced into LDS, then each thread sums its trace in node order.
//     tile role   P_sr in compressed sparse blocks: traces cut in tiles of 2^tshift, the tile's
//                 q_k staged in LDS with coalesced loads, and each (tile, op) pair -- the op's
//                 traces inside the tile as u16 tile-local indices -- summed in trace order
//                 (a thread per short pair, a wave per long one) into part[pair].
//   k_iter_b, a wave per op: s'[o] = d * (sum of the op's pair partials in tile order / M_r(k)
//                 + alpha * sum_{p in ss(o)} pw_p * s_k[p] / M_s(k))                 (:122-124)
// The op side never gathers q from HBM at random (an op-major CSC did: 5% of HBM at 10M
// traces).  Maxima M_s, M_r (np.amax, :126-127) travel as bit patterns of non-negative doubles
// through atomicMax (exact, order-independent).  Normalisation of r is deferred:
// sum_t w_t (r'_t / M_r) is evaluated as (sum_t w_t r'_t) / M_r.  Every float reduction has a
// fixed order (no float atomics), so results are bitwise reproducible run to run.
//
// For graphs with N <= FX_NMAX and P_rs == P_sr (every graph built from spans): ONE read of the
// trace-major u16 ids per iteration serves both products of pagerank.py:122-125.
//   k_tr_a  lane = trace (wave tiles of 64 traces, below):
//     r'[t]   = d * sum_{o in ops(t)} su_k[o] / M_s(k) + fp32((1-d) v_t)        (layout order)
//     lacc[o] += X_t for o in ops(t),   X_t = rint(w_t r'_k[t] / M_r(k) * 2^SC)   (LDS, u64)
//   The block's N accumulators go out as one dense row part[block][0..N).  Because X_t <= 2^SC
//   (w_t <= 1, r'_k <= M_r(k)) and SC = 64 - bits(traces of the block), a row entry stays < 2^64.
//   k_fx_b  wave per op: S_o = sum over blocks of part[.][o] as two exact 32-bit-limb sums, one
//   rounding to double, then s'[o] = d * (S_o 2^-SC + alpha * sum_p pw_p s_k[p] / M_s(k)).
// Integer sums are exact, so the result does not depend on atomic or reduction order: runs are
// bitwise reproducible, and the quantisation (2^-SC absolute per term, SC >= 53) sits below
// fp64's own rounding of the reference's dot products.
//
// This unit: the iteration's launches (iterate, iterate_to_tol), the ranking attempt around them
// (pagerank_attempt: check, set-up, plan and cut -- mr_pr_plan.hip --, describe -- mr_pr_launch.hip --,
// iterate, weights, error words) and every public entry.  The kernels live in units of their own
// (mr_pr_walk.hip, mr_pr_fxb.hip, mr_pr_tile_cold.hip); only k_weights_batch is here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "mr_pr_iter.h"
#include "mr_prim.h"

namespace {

// result = s/max(s) (pagerank.py:126,129); weight = result * sum(result) / N (:93-107)
// (one block of up to 1024 threads per graph)
__device__ __forceinline__ void weights_body(const double* sp, const unsigned long long* mslot, int k3, int32_t N,
                                             int exact, double* sn, double* weight, double* scal) {
    __shared__ double red[1024 / WAVE];
    __shared__ double tot;
    double ms = -__builtin_huge_val();
    for (int i = threadIdx.x; i < MSH; i += blockDim.x) ms = nmax(ms, bits2d(mslot[(size_t)2 * MSH * k3 + i]));
    const double Ms = block_max(ms, red);
    double m = -__builtin_huge_val();
    for (int32_t o = threadIdx.x; o < N; o += blockDim.x) {
        double v = sp[o] / Ms;
        sn[o] = v;
        m = nmax(m, v);
    }
    m = block_max(m, red);
    for (int32_t o = threadIdx.x; o < N; o += blockDim.x) sn[o] = sn[o] / m;
    __syncthreads();
    if (exact) {
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int32_t o = 0; o < N; ++o) s += sn[o];
            tot = s;
        }
        __syncthreads();
    } else {
        int32_t per = (N + blockDim.x - 1) / blockDim.x;
        int32_t a = threadIdx.x * per, b = min(a + per, N);
        double s = 0.0;
        for (int32_t o = a; o < b; ++o) s += sn[o];
        s = block_sum(s, red);
        if (threadIdx.x == 0) tot = s;
        __syncthreads();
    }
    const double total = tot;
    for (int32_t o = threadIdx.x; o < N; o += blockDim.x) weight[o] = sn[o] * total / (double)N;
    if (threadIdx.x == 0) scal[4] = total;
}
// the weights of every graph of a batch (block g: graph g) plus a gather of each graph's four error
// words into one buffer, so the call's single read-back is one pinned copy
__global__ void __launch_bounds__(1024) k_weights_batch(const GDev* __restrict__ gs, int iters, int exact,
                                                        int32_t* flags_out) {
    const GDev& G = gs[blockIdx.x];
    if (threadIdx.x < 4) flags_out[4 * blockIdx.x + threadIdx.x] = G.flag[threadIdx.x];
    weights_body(G.spb[iters & 1], G.mslot, iters % 3, G.N, exact, G.sn, G.weight, G.scal);
}
}  // namespace

// ------------------------------------------------------------------------------ host side
void mr_prof_begin(mr_ctx* ctx);
void mr_prof_end(mr_ctx* ctx, double bytes, int64_t iters = 1);

// ---- the steps of one attempt, in pagerank_attempt's order

// the arguments, before any device work
static int attempt_check(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, int iters, bool sharded) {
    if (!ctx || ng <= 0 || !gs || !anomaly) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank: bad arguments");
    if (iters < 0) return mr_fail(ctx, MR_ERR_ARG, "iters < 0");
    for (int i = 0; i < ng; ++i) {
        if (!gs[i] || gs[i]->ctx != ctx) return mr_fail(ctx, MR_ERR_STATE, "mr_pagerank: bad handles");
        // np.amax of an empty vector (pagerank.py:126-127); a shard tests the whole graph's traces,
        // so a rank whose shard is empty still joins every collective of the call
        const int64_t T = sharded ? gs[i]->T_all : (int64_t)gs[i]->T;
        if (gs[i]->N == 0 || T == 0)
            return mr_fail(ctx, MR_ERR_VALUE, "zero-size array to reduction operation maximum which has no identity");
    }
    return MR_OK;
}

// set-up of every graph not set up ahead (mr_pagerank_presetup): batched when they allow it
// setup_h / setup_d: the batched set-up's descriptors, alive until the call's final sync
static int attempt_setup(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, bool fp32,
                         uint32_t flags, bool sharded, uint64_t seed, uint64_t hmask,
                         std::vector<unsigned char>& setup_h, DBuf<unsigned char>& setup_d) {
    std::vector<mr_graph*> need;
    std::vector<int> need_a;
    bool batch = !sharded && getenv("MR_NO_SETUP_BATCH") == nullptr;
    for (int i = 0; i < ng; ++i) {
        mr_graph* g = gs[i];
        const bool pre = g->pre_ok && g->pre_anomaly == anomaly[i] && g->pre_d == d && g->pre_phi == g->phi && g->pre_fp32 == fp32 &&
                         g->pre_flags == flags && g->pre_seed == seed && g->pre_hmask == hmask && !sharded;
        g->pre_ok = false;   // the iteration state is consumed by this call
        g->rk_ok = g->trank_ok = false;   // ... and the last ranking's is overwritten
        if (pre) continue;
        need.push_back(g);
        need_a.push_back(anomaly[i]);
        batch = batch && setup_batchable(g, flags);
    }
    if (batch && need.size() >= 2)
        return pagerank_setup_batch(ctx, need.data(), need_a.data(), (int)need.size(), d, fp32, seed, hmask, setup_h,
                                    setup_d);
    for (size_t j = 0; j < need.size(); ++j)
        MR_TRY(pagerank_setup(ctx, need[j], need_a[j], d, fp32, flags, sharded, seed, hmask));
    return MR_OK;
}

// a sharded wide graph: the widest cold slice span over the ranks (one scale for every rank)
static int cold_span_over_ranks(mr_ctx* ctx, mr_graph* const* gs, int ng, bool sharded, uint64_t* cold_span_all) {
    *cold_span_all = 1;
    for (int i = 0; i < ng; ++i)
        if (gs[i]->wide) *cold_span_all = std::max(*cold_span_all, gs[i]->cold_span);
    if (sharded && mr_coll_ready(ctx)) {
        DBuf<uint64_t> csp;
        MR_TRY(csp.upload(ctx, cold_span_all, 1));
        MR_TRY(mr_coll_allreduce(ctx, csp.p, 1, MR_DT_U64, 1));
        MR_TRY(csp.download(ctx, cold_span_all, 1));
        MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MR_OK;
}

// The power iteration: per iteration the wide graphs' cold halves, k_tr_a + k_fx_b for the fused graphs
// and k_iter_a + k_iter_b for the others, a sharded graph's all-reduce between each pair's halves
// Iterations [it_begin, it_end) of the call; cv: the residual of each goes to its history (k_resid,
// outside the roofline bracket)
static int iterate(mr_ctx* ctx, mr_graph* const* gs, int ng, bool fp32, double d, double alpha, int it_begin, int it_end,
                   const FxPlan& plan, const std::vector<GDev>& hv, const GDev* dv, Launch& L,
                   const Converge* cv = nullptr) {
    hipStream_t st = ctx->stream, sst = L.sst;
    const bool side = L.any_wide && sst != st;
    // (the kernels of the other units, as host function pointers)
    const ColdOps cold_ops = cold_ops_kernel(fp32);
    const ColdTrace cold_trace = cold_trace_kernel();
    const IterA iter_a = iter_a_kernel(fp32);
    const IterB iter_b = iter_b_kernel();
    const FxB fx_b_k = fx_b_kernel(L.fb_small);
    const int fb_threads = WAVE * (L.fb_small ? FB_W_SMALL : FB_W);
    for (int it = it_begin; it < it_end; ++it) {
        mr_prof_begin(ctx);
        if (side) {
            MR_TRY_HIP(ctx, hipEventRecord(ctx->side_ev[0], st));   // this iteration's su and q are ready
            MR_TRY_HIP(ctx, hipStreamWaitEvent(sst, ctx->side_ev[0], 0));
        }
        for (int i = 0; i < ng; ++i) {   // wide graphs: the cold halves, before k_tr_a / k_fx_b
            mr_graph* g = gs[i];
            if (!g->wide) continue;
            const void* qc = fp32 ? (const void*)g->q32[it & 1].p : (const void*)g->q64[it & 1].p;
            const size_t lds_c = (size_t)g->cold_rw * sizeof(unsigned long long);
            hipLaunchKernelGGL(cold_ops, dim3(g->n_cb), dim3(WIDE_CT), lds_c, sst, g->cb_beg.p, g->cp_pos.p, g->cp_op.p,
                               qc, g->mslot.p, it, hv[(size_t)i].cx_scale, g->cold_rw, (unsigned long long*)g->cold_part.p);
            // (the listed tiles only: the short-tile walk gathers the rest itself; cold_all: every tile)
            const int32_t ntl = L.cold_all ? g->n_wt : g->n_ctl;
            if (ntl)
                hipLaunchKernelGGL(cold_trace, dim3(cdiv((int64_t)ntl * WAVE, 256)), dim3(256), 0, st,
                                   g->cold_off_p.p, g->cold_ops_p.p, g->sub[it & 1].p,
                                   L.cold_all ? (const int32_t*)nullptr : g->ctl.p, ntl, g->T, g->cold_acc.p);
            MR_DEBUG_CHECK(ctx, "k_cold");
        }
        if (side) MR_TRY_HIP(ctx, hipEventRecord(ctx->side_ev[1], sst));
        if (L.blocks_fa) {
            hipLaunchKernelGGL(L.tr_a, dim3(L.blocks_fa), dim3(plan.NT), L.lds_f, st, dv, ng, L.split_fa, d, alpha, it, 0);
            MR_DEBUG_CHECK(ctx, "k_tr_a");
            if (side) MR_TRY_HIP(ctx, hipStreamWaitEvent(st, ctx->side_ev[1], 0));   // k_cold_ops done
            auto fx_b = [&](int mode, const MrPeerX& p) {
                hipLaunchKernelGGL(fx_b_k, dim3(L.blocks_fb), dim3(fb_threads), 0, st, dv, ng, L.split_fb, d, it, mode, p);
            };
            if (!L.coll) {
                // (none: every graph finished by its last k_tr_a block; pf launches: the next k_tr_a
                // finishes this iteration, k_fx_b only after the last one)
                if (L.blocks_fb && (!L.launch_pf || it == it_end - 1)) fx_b(0, L.px_off);
            } else if (L.px_on) {   // the exchange fused into k_fx_b: push in mode 1, per-block waits in mode 2
                fx_b(1, L.px);
                if (!L.px.spin) MR_TRY(mr_peer_fx_wait(ctx, L.px, L.blocks_fb));
                fx_b(2, L.px);
                mr_peer_fx_round_done(ctx, &L.px);
            } else {   // ONE all-reduce: the P_sr r limbs and every rank's r' max (exact: integers)
                fx_b(1, L.px_off);
                const int64_t nw = 2 * (int64_t)gs[0]->N + ctx->nranks;
                const int prc = mr_peer_allreduce_u64(ctx, (unsigned long long*)gs[0]->fx_limb.p, nw);
                if (prc == MR_ERR_STATE) MR_TRY(mr_coll_allreduce(ctx, gs[0]->fx_limb.p, nw, MR_DT_U64, 0));
                else MR_TRY(prc);
                fx_b(2, L.px_off);
            }
            MR_DEBUG_CHECK(ctx, "k_fx_b");
        }
        if (L.blocks_a) {
            hipLaunchKernelGGL(iter_a, dim3(L.blocks_a), dim3(TB), L.lds, st, dv, ng, d, it);
            MR_DEBUG_CHECK(ctx, "k_iter_a");
        }
        if (L.blocks_b) {
            if (!L.coll) {
                hipLaunchKernelGGL(iter_b, dim3(L.blocks_b), dim3(TB), 0, st, dv, ng, d, alpha, it, 0);
            } else {   // ONE all-reduce: the per-op P_sr r sums (fp64 SUM) and every rank's r' max
                hipLaunchKernelGGL(iter_b, dim3(L.blocks_b), dim3(TB), 0, st, dv, ng, d, alpha, it, 1);
                const int64_t nw = (int64_t)gs[0]->N + ctx->nranks;
                const int prc = mr_peer_allreduce_f64(ctx, gs[0]->op_sum.p, nw);
                if (prc == MR_ERR_STATE) MR_TRY(mr_coll_allreduce(ctx, gs[0]->op_sum.p, nw, MR_DT_F64, 0));
                else MR_TRY(prc);
                hipLaunchKernelGGL(iter_b, dim3(L.blocks_b), dim3(TB), 0, st, dv, ng, d, alpha, it, 2);
            }
            MR_DEBUG_CHECK(ctx, "k_iter_b");
        }
        mr_prof_end(ctx, L.bytes);
        if (cv) {
            mr_resid_launch(ctx, dv, ng, L.blocks_r, it, cv->max_iters, it, false, cv->resid_dev);
            MR_DEBUG_CHECK(ctx, "k_resid");
        }
    }
    return MR_OK;
}

// The iterations of a convergence request: stretches of check_every iterations (one stretch of
// max_iters when tol == 0), after each the history so far copied to the host (pinned words when
// it fits them) with the call's only syncs before the closing one
static int iterate_to_tol(mr_ctx* ctx, mr_graph* const* gs, int ng, bool fp32, double d, double alpha, const FxPlan& plan,
                          const std::vector<GDev>& hv, const GDev* dv, Launch& L, Converge* cv) {
    const size_t bytes = (size_t)ng * (size_t)cv->max_iters * sizeof(double);
    MR_TRY_HIP(ctx, hipMemsetAsync(cv->resid_dev, 0, bytes, ctx->stream));   // (a retry overwrites the history)
    int it = 0;
    while (it < cv->max_iters) {
        const int end = cv->tol > 0.0 ? std::min(it + cv->check_every, cv->max_iters) : cv->max_iters;
        MR_TRY(iterate(ctx, gs, ng, fp32, d, alpha, it, end, plan, hv, dv, L, cv));
        // (one graph: the stretch's words are contiguous.  The fallback collective, not the peer regions)
        if (cv->agree) MR_TRY(mr_coll_allreduce(ctx, cv->resid_dev + it, end - it, MR_DT_U64, 1));
        it = end;
        if (bytes <= MR_PIN_BYTES) {
            unsigned char* hp = nullptr;
            MR_TRY(mr_read_bytes(ctx, cv->resid_dev, bytes, &hp));
            memcpy(cv->resid, hp, bytes);
        } else {
            MR_TRY_HIP(ctx, hipMemcpyAsync(cv->resid, cv->resid_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
            MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        bool all = true;   // (a NaN residual compares false: such a graph never counts as converged)
        for (int i = 0; i < ng; ++i) all = all && cv->resid[(size_t)i * cv->max_iters + (it - 1)] <= cv->tol;
        if (all) break;
    }
    cv->iters_done = it;
    return MR_OK;
}

// The error words of ng graphs (4 per graph: kind-hash collision, division by zero, partition
// overflow), graph by graph: a collision makes the caller retry with the next seed
static int decode_error_words(mr_ctx* ctx, const int32_t* words, const int* anomaly, int ng, bool* collided) {
    *collided = false;
    for (int i = 0; i < ng; ++i) {
        const int32_t* w = words + 4 * (size_t)i;
        *collided = w[0] & 1;
        if (*collided) return MR_OK;
        if (w[2] & 1) return mr_fail(ctx, MR_ERR_STATE, "trace kinds: a partition exceeded its table");
        if (anomaly[i] && (w[1] & 1)) return mr_fail(ctx, MR_ERR_ZERODIV, "float division by zero");
    }
    return MR_OK;
}

// One attempt with kind-hash seed `seed`; *collided reports a 64-bit key collision found by the
// exact verification (k_kind_verify / k_sh_kind_check), after which the caller retries.
// as: enqueue only (window groups); mr_pagerank_async_finish reads the error words
// cv: a convergence request (iters = its max_iters; never with `as`) -- no pf
// launches: the next launch's prologue would finish an iteration and then clear the ring slot the
// residual reads; the k_fx_b form's results are bitwise the pf form's.  On a shard (cv->agree) k_resid
// runs unchanged: k_fx_b / k_iter_b mode 2 leave spb[(it+1)&1] and the s half of ring slot (it+1)%3
// replicated on every rank, and the words still meet in a MAX before they are read
// last_resid ([ng] host; as: as->report): the residual of the last iteration alone, one k_resid
// behind the iterations, in every launch form -- nothing runs after the closing k_fx_b, so the ring
// slots and both vectors it reads are intact; its words share the error words' read
static int pagerank_attempt(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, double alpha,
                            int iters, int precision, uint32_t flags, bool sharded, uint64_t seed, uint64_t hmask,
                            bool* collided, PrAsync* as = nullptr, Converge* cv = nullptr, double* last_resid = nullptr) {
    *collided = false;
    HostMarks hm(ng);
    MR_TRY(attempt_check(ctx, gs, anomaly, ng, iters, sharded));
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool fp32 = precision == MR_FP32;
    PrAsync own;   // what the kernels read lives until the final sync of a call that waits, else in the caller's `as`
    PrAsync& s = as ? *as : own;
    MR_TRY(attempt_setup(ctx, gs, anomaly, ng, d, fp32, flags, sharded, seed, hmask, s.setup_h, s.setup_d));
    hm.mark("setup");
    const FxPlan plan = fx_plan(gs, ng, fp32, sharded, cv == nullptr);
    std::vector<int64_t> nfa;
    MR_TRY(cut_blocks(ctx, gs, ng, plan, hm, nfa));   // (marks "blocks" before its launches)
    uint64_t cold_span_all = 1;
    MR_TRY(cold_span_over_ranks(ctx, gs, ng, sharded, &cold_span_all));
    // ---- batched power iteration: one k_tr_a (+ k_fx_b) or k_iter_a + k_iter_b per iteration for every graph
    s.hv = std::vector<GDev>((size_t)ng);   // (value-initialised: the kernels read the fields a path leaves out as 0)
    const TrKnobs kn;
    Launch L;
    int64_t fb16 = 0;   // k_fx_b blocks of the launch at 16 ops per block
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused) fb16 += cdiv(gs[i]->N, 16);
    for (int i = 0; i < ng; ++i) {
        GDev& v = s.hv[(size_t)i];
        gdev_pointers(v, ctx, gs[i], fp32, alpha, plan);
        gdev_scales(v, gs[i], sharded, cold_span_all);
        gdev_launch(v, gs[i], nfa[(size_t)i], fp32, sharded, plan, kn, fb16 > FB_MANY_BLOCKS, L);
    }
    MR_TRY(finalise_launch(ctx, gs, ng, fp32, sharded, plan, kn, s.hv, L));
    hm.mark("descr");
    MR_TRY(s.dv.upload(ctx, s.hv.data(), s.hv.size()));
    MR_TRY(prepare_exchange(ctx, gs, ng, L));
    hm.mark("pre-loop");
    if (cv) {
        MR_TRY(iterate_to_tol(ctx, gs, ng, fp32, d, alpha, plan, s.hv, s.dv.p, L, cv));
        iters = cv->iters_done;   // (k_weights_batch: spb[iters & 1], ring slot iters % 3)
    } else {
        MR_TRY(iterate(ctx, gs, ng, fp32, d, alpha, 0, iters, plan, s.hv, s.dv.p, L));
    }
    // weights of every graph and the gathered error words in one launch (the flags are final:
    // the kernels that raise them ran before the iterations; a sharded graph's words meet in a
    // MAX first, below, so it reads them after that)
    DBuf<int32_t>& fl = s.fl;
    const bool report = !cv && !sharded && iters >= 1 && (as ? as->report : last_resid != nullptr);
    const size_t nwords = (size_t)(report ? 6 : 4) * ng;   // (a report: 8-byte residual words behind the error words)
    MR_TRY(fl.alloc(ctx, nwords));
    hm.mark("loop");
    if (report) {
        unsigned long long* rw = (unsigned long long*)(fl.p + (size_t)4 * ng);
        const bool one_block = L.blocks_r == ng;   // (window graphs: N <= RESID_OPS) each block stores its word
        if (!one_block) MR_TRY_HIP(ctx, hipMemsetAsync(rw, 0, (size_t)ng * sizeof(unsigned long long), st));
        mr_resid_launch(ctx, s.dv.p, ng, L.blocks_r, iters - 1, 1, 0, one_block, rw);
        MR_DEBUG_CHECK(ctx, "k_resid");
    }
    hipLaunchKernelGGL(k_weights_batch, dim3(ng), dim3(1024), 0, st, s.dv.p, iters,
                       (int)((flags & MR_PR_EXACT_SUMS) != 0), fl.p);
    MR_DEBUG_CHECK(ctx, "k_weights_batch");
    MR_TRY_HIP(ctx, hipGetLastError());
    if (L.coll && ctx->peer_on) MR_TRY(mr_peer_check(ctx, "peer all-reduce"));   // an error, not wrong sums
    // a shard's local collision must make every rank retry: the error words meet in a MAX
    if (L.coll) {
        MR_TRY(mr_coll_allreduce(ctx, gs[0]->flag.p, 4, MR_DT_I32, 1));
        MR_TRY_HIP(ctx, hipMemcpyAsync(fl.p, gs[0]->flag.p, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    if (as) {   // enqueued only: the words go to the caller's pinned slot, the finish reads them
        as->anomaly.assign(anomaly, anomaly + ng);
        as->ng = ng;
        return as->defer ? MR_OK : mr_pagerank_async_commit(ctx, as);
    }
    // the only host round trip of the call: error words raised by the kernels (one pinned read)
    std::vector<int32_t> hflag(nwords, 0);
    if (nwords * sizeof(int32_t) <= MR_PIN_BYTES) {
        unsigned char* hp = nullptr;
        MR_TRY(mr_read_bytes(ctx, fl.p, nwords * sizeof(int32_t), &hp));
        memcpy(hflag.data(), hp, hflag.size() * sizeof(int32_t));
    } else {
        MR_TRY(fl.download(ctx, hflag.data(), hflag.size()));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    }
    if (report) memcpy(last_resid, hflag.data() + (size_t)4 * ng, (size_t)ng * sizeof(double));
    MR_TRY(decode_error_words(ctx, hflag.data(), anomaly, ng, collided));
    if (!*collided)   // what this ranking left on the device: q[iters & 1], ring slot iters % 3 (mr_exemplar.hip)
        for (int i = 0; i < ng; ++i) {
            gs[i]->rk_ok = true;
            gs[i]->rk_fp32 = fp32;
            gs[i]->rk_kc = false;
            gs[i]->rk_sharded = sharded;
            gs[i]->rk_iters = iters;
            gs[i]->rk_d = d;
        }
    return MR_OK;
}

int mr_pagerank_batch_impl(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, double alpha,
                           int iters, int precision, uint32_t flags, bool sharded, double* last_resid) {
    constexpr int ATTEMPTS = 4;
    for (int a = 0; a < ATTEMPTS; ++a) {
        bool collided = false;
        MR_TRY(pagerank_attempt(ctx, gs, anomaly, ng, d, alpha, iters, precision, flags, sharded, kind_seed(a),
                                kind_hmask(a), &collided, nullptr, nullptr, last_resid));
        if (!collided) return MR_OK;
    }
    return mr_fail(ctx, MR_ERR_STATE, "trace-kind hash collision under %d seeds", ATTEMPTS);
}

extern "C" int mr_pagerank(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters,
                           int precision, uint32_t flags) {
    if (g) g->phi = 0.5;
    if (flags & MR_PR_KIND_COMPRESS) return kind_compressed_call(ctx, g, anomaly, d, alpha, iters, precision, flags);
    return mr_pagerank_batch_impl(ctx, &g, &anomaly, 1, d, alpha, iters, precision, flags);
}

extern "C" int mr_pagerank_ex(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters, double phi,
                              int precision, uint32_t flags) {
    if (!g || !(phi > 0.0)) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_ex: bad graph or phi");
    g->phi = phi;
    const int rc = (flags & MR_PR_KIND_COMPRESS) ? kind_compressed_call(ctx, g, anomaly, d, alpha, iters, precision, flags)
                                                 : mr_pagerank_batch_impl(ctx, &g, &anomaly, 1, d, alpha, iters, precision, flags);
    g->phi = 0.5;
    return rc;
}

int mr_pagerank_async_commit(mr_ctx* ctx, PrAsync* a) {
    MR_TRY_HIP(ctx, hipMemcpyAsync(a->hflag, a->fl.p, (size_t)(a->report ? 6 : 4) * a->ng * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, ctx->stream));
    if (!a->ev) MR_TRY_HIP(ctx, hipEventCreateWithFlags(&a->ev, hipEventDisableTiming));
    MR_TRY_HIP(ctx, hipEventRecord(a->ev, ctx->stream));
    a->committed = true;
    return MR_OK;
}
int mr_pagerank_batch_async(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, double alpha,
                            int iters, int precision, int32_t* hflag, PrAsync** out, bool defer, bool report) {
    std::unique_ptr<PrAsync> a(new PrAsync());
    a->hflag = hflag;
    a->defer = defer;
    a->report = report && iters >= 1;
    bool collided = false;
    MR_TRY(pagerank_attempt(ctx, gs, anomaly, ng, d, alpha, iters, precision, 0, false, kind_seed(0), kind_hmask(0),
                            &collided, a.get()));
    *out = a.release();
    return MR_OK;
}
int mr_pagerank_async_finish(mr_ctx* ctx, PrAsync* a, bool* rerun) {
    *rerun = false;
    if (!a->committed) MR_TRY(mr_pagerank_async_commit(ctx, a));   // (a deferred batch nobody committed)
    MR_TRY_HIP(ctx, hipEventSynchronize(a->ev));
    return decode_error_words(ctx, a->hflag, a->anomaly.data(), a->ng, rerun);   // (a collision: the caller reruns)
}
const double* mr_pagerank_async_resid(const PrAsync* a) {
    return a->report ? (const double*)(a->hflag + (size_t)4 * a->ng) : nullptr;
}
void mr_pagerank_async_free(PrAsync* a) { delete a; }

extern "C" int mr_pagerank_batch(mr_ctx* ctx, mr_graph* const* graphs, const int* anomaly, int n_graphs, double d,
                                 double alpha, int iters, int precision, uint32_t flags) {
    return mr_pagerank_batch_impl(ctx, graphs, anomaly, n_graphs, d, alpha, iters, precision, flags);
}

// mr_pagerank_batch that records every iteration's residual and may stop at a tolerance
// (README.md:37; pagerank.py:117's fixed count).  A kind-hash collision reruns the attempt, history included.
extern "C" int mr_pagerank_converge(mr_ctx* ctx, mr_graph* const* graphs, const int* anomaly, int n_graphs, double d,
                                    double alpha, int max_iters, double phi, int precision, uint32_t flags, double tol,
                                    int check_every, int32_t* iters_done, double* resid, int32_t* converged_at) {
    if (!ctx || !graphs || !anomaly || n_graphs <= 0 || !iters_done || !resid)
        return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_converge: bad arguments");
    if (max_iters < 1 || check_every < 1) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_converge: max_iters, check_every < 1");
    if (!(tol >= 0.0)) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_converge: tol negative or NaN");
    if (!(phi > 0.0)) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_converge: phi <= 0");
    if (flags & MR_PR_KIND_COMPRESS)
        return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_converge: MR_PR_KIND_COMPRESS is not supported");
    for (int i = 0; i < n_graphs; ++i) {
        if (!graphs[i] || graphs[i]->ctx != ctx) return mr_fail(ctx, MR_ERR_STATE, "mr_pagerank: bad handles");
        if (graphs[i]->shard_built)
            return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_converge: a graph of mr_graph_build_sharded is not supported");
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nw = (size_t)n_graphs * (size_t)max_iters;
    DBuf<unsigned long long> rd;
    MR_TRY(rd.alloc(ctx, nw));
    Converge cv{tol, check_every, max_iters, rd.p, resid, 0};
    for (int i = 0; i < n_graphs; ++i) graphs[i]->phi = phi;
    constexpr int ATTEMPTS = 4;   // (mr_pagerank_batch_impl's seed sequence)
    int rc = MR_OK;
    bool collided = true;
    for (int a = 0; a < ATTEMPTS && rc == MR_OK && collided; ++a)
        rc = pagerank_attempt(ctx, graphs, anomaly, n_graphs, d, alpha, max_iters, precision, flags, false, kind_seed(a),
                              kind_hmask(a), &collided, nullptr, &cv);
    for (int i = 0; i < n_graphs; ++i) graphs[i]->phi = 0.5;
    MR_TRY(rc);
    if (collided) return mr_fail(ctx, MR_ERR_STATE, "trace-kind hash collision under %d seeds", ATTEMPTS);
    *iters_done = cv.iters_done;
    if (converged_at)
        for (int i = 0; i < n_graphs; ++i) {
            converged_at[i] = -1;
            for (int k = 0; k < cv.iters_done && converged_at[i] < 0; ++k)
                if (resid[(size_t)i * max_iters + k] <= tol) converged_at[i] = k + 1;
        }
    return MR_OK;
}

// The synchronous ranking of a window group (mr_internal.h): mr_pagerank_batch with the call's count and
// the last iteration's residuals, or the convergence attempt, whose history stays here
int mr_pagerank_batch_report(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, double alpha,
                             int iters, int precision, double tol, int check_every, int32_t* iters_done, double* resid) {
    if (!(tol > 0.0)) {
        MR_TRY(mr_pagerank_batch_impl(ctx, gs, anomaly, ng, d, alpha, iters, precision, 0, false, resid));
        *iters_done = iters;
        return MR_OK;
    }
    if (ng <= 0 || iters < 1 || check_every < 1) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_batch_report: bad arguments");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nw = (size_t)ng * (size_t)iters;
    DBuf<unsigned long long> rd;
    MR_TRY(rd.alloc(ctx, nw));
    std::vector<double> hist(nw, 0.0);
    Converge cv{tol, check_every, iters, rd.p, hist.data(), 0};
    constexpr int ATTEMPTS = 4;   // (mr_pagerank_batch_impl's seed sequence)
    bool collided = true;
    for (int a = 0; a < ATTEMPTS && collided; ++a)
        MR_TRY(pagerank_attempt(ctx, gs, anomaly, ng, d, alpha, iters, precision, 0, false, kind_seed(a), kind_hmask(a),
                                &collided, nullptr, &cv));
    if (collided) return mr_fail(ctx, MR_ERR_STATE, "trace-kind hash collision under %d seeds", ATTEMPTS);
    *iters_done = cv.iters_done;
    if (resid)
        for (int i = 0; i < ng; ++i) resid[i] = hist[(size_t)i * iters + (cv.iters_done - 1)];
    return MR_OK;
}

// What a sharded ranking needs before its attempt: the graph-level exchange (once per graph) and the
// per-iteration all-reduce buffer.  Collective.
static int sharded_prologue(mr_ctx* ctx, mr_graph* g) {
    if (!mr_coll_ready(ctx) && ctx->nranks != 1) return mr_fail(ctx, MR_ERR_COMM, "no collective backend");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (!g->sharded_done) {   // the graph-level exchange happens once per graph
        if (mr_coll_ready(ctx) && ctx->nranks > 1) {
            // every rank must run the same iteration (the fused path's u64 limb all-reduce or the
            // tile path's fp64 op sums): the fused choice depends on this shard (e.g. a trace
            // without ops), so the ranks agree on it -- fused only if fused everywhere
            DBuf<int32_t> f;
            int32_t tile = g->fused ? 0 : 1;   // MAX over ranks: 1 if any rank takes the tile path
            MR_TRY(f.upload(ctx, &tile, 1));
            MR_TRY(mr_coll_allreduce(ctx, f.p, 1, MR_DT_I32, 1));
            MR_TRY(f.download(ctx, &tile, 1));
            MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (g->fused && tile) {
                g->force_tile = true;
                MR_TRY(mr_graph_prepare(ctx, g));   // the P_sr tiles (before the per-op sums below)
            }
        }
        MR_TRY(shard_exchange(ctx, g));
        g->sharded_done = true;
    }
    // the per-iteration all-reduce buffer: the per-op sums, then one r' max slot per rank
    if (g->fused) MR_TRY(g->fx_limb.alloc(ctx, 2 * (size_t)g->N + (size_t)ctx->nranks));   // fixed-point limbs
    else MR_TRY(g->op_sum.alloc(ctx, (size_t)g->N + (size_t)ctx->nranks));                  // tile path: fp64 sums
    return MR_OK;
}

extern "C" int mr_pagerank_sharded(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters,
                                   int precision, uint32_t flags) {
    if (!ctx || !g || g->ctx != ctx) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded: bad handles");
    MR_TRY(sharded_prologue(ctx, g));
    return mr_pagerank_batch_impl(ctx, &g, &anomaly, 1, d, alpha, iters, precision, flags, true);
}

// mr_pagerank_sharded with mr_pagerank_converge's history and stop (README.md:37; pagerank.py:117's
// fixed count).  The ranks first compare their requests (a differing count of checks would hang them),
// then agree on every check's words (Converge::agree).
extern "C" int mr_pagerank_sharded_converge(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int max_iters,
                                            double phi, int precision, uint32_t flags, double tol, int check_every,
                                            int32_t* iters_done, double* resid, int32_t* converged_at) {
    if (!ctx || !g || g->ctx != ctx || !iters_done || !resid)
        return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded_converge: bad handles or null arguments");
    if (!mr_coll_ready(ctx) && ctx->nranks != 1) return mr_fail(ctx, MR_ERR_COMM, "no collective backend");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const int R = ctx->nranks;
    if (mr_coll_ready(ctx) && R > 1) {   // the same request on every rank, before anything depends on it
        constexpr int NW = 9;
        auto bits = [](double x) { uint64_t b; memcpy(&b, &x, sizeof b); return b; };
        const uint64_t mine[NW] = {(uint64_t)(int64_t)max_iters, (uint64_t)(int64_t)check_every, bits(tol), bits(d), bits(alpha),
                                   bits(phi), (uint64_t)(int64_t)precision, (uint64_t)flags, (uint64_t)(anomaly != 0)};
        DBuf<uint64_t> send, recv;
        std::vector<uint64_t> all((size_t)NW * R);
        MR_TRY(send.upload(ctx, mine, NW));
        MR_TRY(recv.alloc(ctx, (size_t)NW * R));
        MR_TRY(mr_coll_allgather(ctx, send.p, recv.p, NW, MR_DT_U64));
        MR_TRY(recv.download(ctx, all.data(), all.size()));
        MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int r = 0; r < R; ++r)
            if (memcmp(all.data() + (size_t)NW * r, all.data(), sizeof mine) != 0)
                return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded_converge: rank %d's request differs from rank 0's "
                               "(max_iters, check_every, tol, d, alpha, phi, precision, flags, anomaly)", r);
    }
    if (max_iters < 1 || check_every < 1)
        return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded_converge: max_iters, check_every < 1");
    if (!(tol >= 0.0)) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded_converge: tol negative or NaN");
    if (!(phi > 0.0)) return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded_converge: phi <= 0");
    if (flags & MR_PR_KIND_COMPRESS)
        return mr_fail(ctx, MR_ERR_ARG, "mr_pagerank_sharded_converge: MR_PR_KIND_COMPRESS is not supported");
    MR_TRY(sharded_prologue(ctx, g));
    DBuf<unsigned long long> rd;
    MR_TRY(rd.alloc(ctx, (size_t)max_iters));
    Converge cv{tol, check_every, max_iters, rd.p, resid, 0, true};
    g->phi = phi;
    constexpr int ATTEMPTS = 4;   // (mr_pagerank_batch_impl's seed sequence)
    int rc = MR_OK;
    bool collided = true;
    for (int a = 0; a < ATTEMPTS && rc == MR_OK && collided; ++a)
        rc = pagerank_attempt(ctx, &g, &anomaly, 1, d, alpha, max_iters, precision, flags, true, kind_seed(a), kind_hmask(a),
                              &collided, nullptr, &cv);
    g->phi = 0.5;
    MR_TRY(rc);
    if (collided) return mr_fail(ctx, MR_ERR_STATE, "trace-kind hash collision under %d seeds", ATTEMPTS);
    *iters_done = cv.iters_done;
    if (converged_at) {
        *converged_at = -1;
        for (int k = 0; k < cv.iters_done && *converged_at < 0; ++k)
            if (resid[k] <= tol) *converged_at = k + 1;
    }
    return MR_OK;
}
