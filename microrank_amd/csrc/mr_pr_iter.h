// What the units of one ranking attempt share on the host side, in pagerank_attempt's order --
// mr_pr_plan.hip (the launch plan and the per-wave cuts), mr_pr_launch.hip (the graphs' descriptors
// and the launch's form), the kernels' units (mr_pr_walk.hip, mr_pr_fxb.hip, mr_pr_tile_cold.hip:
// each hands its kernels out as host function pointers, as nothing here is built with relocatable
// device code) and mr_pagerank.hip (the iteration and the entries) -- and nobody else.
#pragma once
#include <chrono>
#include <utility>
#include <vector>

#include "mr_iter_dev.h"
#include "mr_pr_internal.h"
#include "mr_pr_walk.h"

// ---------------------------------------------------------------- the attempt's records
// MR_PR_HOST_TIMING: host wall time of pagerank_attempt's phases (no syncs added; diagnostics only)
struct HostMarks {
    bool on = getenv("MR_PR_HOST_TIMING") != nullptr;
    int ng;
    std::vector<std::pair<const char*, std::chrono::steady_clock::time_point>> m;
    explicit HostMarks(int n) : ng(n) { mark("start"); }
    void mark(const char* name) {
        if (on) m.emplace_back(name, std::chrono::steady_clock::now());
    }
    ~HostMarks() {
        if (m.size() < 2) return;
        fprintf(stderr, "[pagerank host ng=%d]", ng);
        for (size_t i = 1; i < m.size(); ++i)
            fprintf(stderr, " %s %.1f", m[i].first, std::chrono::duration<double, std::micro>(m[i].second - m[i - 1].second).count());
        fprintf(stderr, " us\n");
    }
};

// Launch plan of the fused iteration (k_tr_a) for a batch of graphs (one kernel variant per launch).
struct FxPlan {
    int NT = 1024;      // block size (16 waves; 512 when the graphs are small)
    int mode = WV_SU_ALL;   // su in LDS for every fused graph of the batch / hot ops / none
    bool sul = true;    // mode == WV_SU_ALL
    bool pf = false;    // window batches: the next launch finishes an iteration (k_tr_a's pf prologue)
    bool w32 = false;   // fp32 wide graphs only: float su and warm labels in LDS (k_tr_a EXT & TR_X_W32)
};

// The launch-form knobs (A/B and tests, read once per attempt), each on unless set to 0
struct TrKnobs {
    bool lastfin = knob_on("MR_TR_LASTFIN");   // 0: k_fx_b for every graph
    bool ssv = knob_on("MR_TR_SSV");           // 0: k_fx_b computes the call-graph terms
    bool lfssv = knob_on("MR_TR_LFSSV");       // 0: last-block graphs read the terms through the chain
    // 0: plain partial-row stores.  Write-through measured C4 rank 0 of 8: 43.1 vs 44.6 us per
    // iteration, C4 whole: within noise (two repeats each)
    bool row_wt = knob_on("MR_TR_ROW_WT");
};

// the kernels as host function pointers (a unit launches another unit's kernel through one)
using TrA = void (*)(const GDev*, int32_t, int32_t, double, double, int, int32_t);                    // k_tr_a
using FxB = void (*)(const GDev*, int32_t, int32_t, double, int, int, const MrPeerX);                 // k_fx_b
using IterA = void (*)(const GDev*, int32_t, double, int);                                            // k_iter_a
using IterB = void (*)(const GDev*, int32_t, double, double, int, int);                               // k_iter_b
using ColdTrace = void (*)(const int32_t*, const int32_t*, const double*, const int32_t*, int32_t, int32_t, double*);
using ColdOps = void (*)(const int64_t*, const int32_t*, const uint16_t*, const void*, const unsigned long long*, int,
                         double, int32_t, unsigned long long*);

// ---------------------------------------------------------------- limits of the launch forms
// FB_W waves per block: 16 for graphs with many partial rows (a large graph alone: ~1k rows per
// op), 4 when every graph of the launch has few (batched window graphs: tens of rows) -- the block
// is then latency-bound (ss term, rows, LDS meet: a chain of dependent loads), and 4-wave blocks
// put the whole grid on the chip in one round instead of several.
constexpr int FB_W = 16, FB_W_SMALL = 4, FB_SMALL_ROWS = 256;
constexpr int64_t FB_MANY_BLOCKS = 1024;   // 16-op blocks of a launch from which "many" holds
constexpr int64_t LASTFIN_WORDS = 32768;   // k_tr_a's last-block finish: partial-row words it reads (256 KB)
constexpr int32_t PF_NMAX = 1024;   // pf launches: ops per graph (three N-word LDS arrays per block)
constexpr int64_t PF_ROWS = 32;     // pf launches: partial rows per graph every block of it sums (C3 windows: up to 19)
#ifndef MR_LF_ONE_CU_LDS
#define MR_LF_ONE_CU_LDS (80 * 1024 + 1024)   // (A/B builds: 0 = every last-block launch takes the acquire)
#endif
constexpr size_t LF_ONE_CU_LDS = MR_LF_ONE_CU_LDS;   // > half of a CU's 160 KB: one block per CU

// What the iteration's launches share: block totals and LDS sizes, summed over the graphs' descriptors
// (gdev_launch), then the launch's variant and streams (finalise_launch, prepare_exchange)
struct Launch {
    int32_t blocks_a = 0, blocks_b = 0, blocks_fa = 0, blocks_fb = 0;   // k_iter_a / k_iter_b / k_tr_a / k_fx_b
    int32_t blocks_r = 0;                   // k_resid (launched only for a convergence request)
    size_t lds = VCAP * sizeof(double), lds_f = 0;   // k_iter_a's / k_tr_a's LDS bytes
    double bytes = 0.0;                     // algorithmic bytes of one iteration (profiling)
    int32_t split_fa = 0, split_fb = 0;     // two graphs: the second one's first block (no search)
    TrA tr_a = nullptr;                     // the k_tr_a variant
    bool launch_pf = false;                 // every graph finishes in-kernel: no k_fx_b before the last iteration
    bool fb_small = false;                  // k_fx_b's block size: 4 waves
    bool coll = false, any_wide = false, px_on = false;
    bool cold_all = false;                  // wide graphs: k_cold_trace over every tile (k_tr_a gathers no cold su)
    hipStream_t sst = nullptr;              // k_cold_ops' stream (the side stream, or the main one)
    MrPeerX px{}, px_off{};                 // the peer exchange inside k_fx_b (px_on), and none
};

// A convergence request (mr_pagerank_converge): the attempt records every iteration's residual
// (k_resid), reads the history every check_every iterations and at max_iters, and stops at the first
// such check K where every graph's resid[K - 1] <= tol.  tol == 0: no intermediate reads.
struct Converge {
    double tol;
    int check_every, max_iters;
    unsigned long long* resid_dev;   // [ng * max_iters] bits of the residuals, zeroed by the attempt
    double* resid;                   // [ng * max_iters] host: the history, entries >= iters_done 0.0
    int iters_done;                  // out: iterations every graph ran
    // a shard (mr_pagerank_sharded_converge): before each read the stretch's words meet in a MAX over
    // the ranks, so every rank reads the same words and takes the same decision
    bool agree = false;
};

// (mr_internal.h) what an enqueued batch's kernels still read, and its error words
struct PrAsync {
    std::vector<unsigned char> setup_h;
    DBuf<unsigned char> setup_d;   // (the batched set-up's descriptors: opaque here)
    std::vector<GDev> hv;
    DBuf<GDev> dv;
    DBuf<int32_t> fl;
    hipEvent_t ev = nullptr;
    int32_t* hflag = nullptr;   // pinned, 4 per graph (6 with a report: the residuals' words behind them)
    bool report = false;        // the last iteration's residual of every graph travels with the words
    std::vector<int> anomaly;
    int ng = 0;
    bool defer = false;         // the words' copy waits for mr_pagerank_async_commit
    bool committed = false;     // the words' copy and the event are enqueued
    ~PrAsync() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

// ---------------------------------------------------------------- mr_pr_plan.hip
FxPlan fx_plan(mr_graph* const* gs, int ng, bool fp32, bool sharded, bool allow_pf = true);
int32_t plan_n_hot(int32_t N, const FxPlan& P);
size_t plan_lds(int32_t N, const FxPlan& P);
int32_t tr_scfix(const mr_graph* g);
int cut_blocks(mr_ctx* ctx, mr_graph* const* gs, int ng, const FxPlan& plan, HostMarks& hm, std::vector<int64_t>& nfa);

// ---------------------------------------------------------------- mr_pr_launch.hip
void gdev_pointers(GDev& v, const mr_ctx* ctx, const mr_graph* g, bool fp32, double alpha, const FxPlan& plan);
void gdev_scales(GDev& v, const mr_graph* g, bool sharded, uint64_t cold_span_all);
void gdev_launch(GDev& v, const mr_graph* g, int64_t nfa, bool fp32, bool sharded, const FxPlan& plan, const TrKnobs& kn,
                 bool fb_many, Launch& L);
int finalise_launch(mr_ctx* ctx, mr_graph* const* gs, int ng, bool fp32, bool sharded, const FxPlan& plan,
                    const TrKnobs& kn, std::vector<GDev>& hv, Launch& L);
int prepare_exchange(mr_ctx* ctx, mr_graph* const* gs, int ng, Launch& L);

// ---------------------------------------------------------------- mr_pr_walk.hip
// the variant of a launch whose fused graphs carry the features `any` (TR_X_KINDS | COLD | RUNS)
int tr_launch_ext(int any, bool w32);
// the k_tr_a built for (precision, su mode, block size, variant); nullptr: not built
TrA tr_kernel(bool fp32, int mode, int NT, int ext);

// ---------------------------------------------------------------- mr_pr_fxb.hip, mr_pr_tile_cold.hip
FxB fx_b_kernel(bool small);   // FB_W_SMALL / FB_W waves per block
IterA iter_a_kernel(bool fp32);
IterB iter_b_kernel();
ColdTrace cold_trace_kernel();
ColdOps cold_ops_kernel(bool fp32);
