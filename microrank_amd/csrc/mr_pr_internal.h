// What the PageRank units share on the host side -- mr_pagerank.hip (the iteration and the public
// entries) and the units of its attempt (mr_pr_plan.hip, mr_pr_launch.hip, mr_pr_walk.hip,
// mr_pr_fxb.hip, mr_pr_tile_cold.hip: what only those share is in mr_pr_iter.h), mr_pr_prepare.hip,
// mr_pr_kinds.hip, mr_pr_setup.hip, mr_pr_shard.hip, and nobody else: the constants two of them
// need, the small helpers, and the functions one unit calls in another.
// Descriptor structs (PDev, SDev, LDev, ...) stay private to their unit.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "mr_internal.h"

// ---------------------------------------------------------------- constants of more than one unit
constexpr int TB = 256;             // trace-role block size (one trace per thread)
constexpr int LONG_PAIR = 32;       // tile pairs longer than this are summed by a whole wave
constexpr int LDS_NODES = 8192;     // k_iter_a: su staged in LDS up to this many nodes (64 KiB)
constexpr int VCAP = 2048;          // k_iter_a: trace-role ids staged per round in LDS (16 KiB of values)
constexpr int WIDE_CT = 1024;       // k_cold_ops block size
constexpr int TR_PAD = WAVE;   // k_tr_a's pad ids N .. N + 63 (su = 0)
constexpr int FX_NMAX = 16384;      // the fused iteration's N (k_tr_a / k_fx_b); wide graphs above
#ifndef MR_WIDE_NA
#define MR_WIDE_NA 10000
#endif
constexpr int32_t WIDE_NA = MR_WIDE_NA;   // (WIDE_NA + TR_PAD) * 16 B + the hot-op sums <= k_tr_a's LDS
#ifndef MR_TR_TIERS512
#define MR_TR_TIERS512 4   // short-tile tiers of the 512-thread k_tr_a (window graphs: occupancy)
#endif
constexpr int TR_TIERS_EXT = 8;   // short-tile tiers of the EXT (kind-compressed / wide) variants
#ifndef MR_TR_TIERS_W32
#define MR_TR_TIERS_W32 5   // ... of the fp32 wide variant (EXT & TR_X_W32: its pipelined cold registers; 6 spilled)
#endif
constexpr int TR_TIERS_W32 = MR_TR_TIERS_W32;
#ifndef MR_HOT_MAX
#define MR_HOT_MAX 8
#endif
constexpr int HOT_MAX = MR_HOT_MAX;
constexpr int HOT_MAX_WIDE = 4;   // wide graphs' k_tr_a variant (its cold registers): 4 accumulators

// ---------------------------------------------------------------- small helpers
// MR_DEBUG=1: check every launch (names the failing kernel instead of a later sticky error)
static const bool g_debug = getenv("MR_DEBUG") != nullptr;
#define MR_DEBUG_CHECK(ctx, name)                                                                          \
    do {                                                                                                   \
        if (g_debug) {                                                                                     \
            hipError_t e_ = hipGetLastError();                                                             \
            if (e_ == hipSuccess) e_ = hipStreamSynchronize((ctx)->stream);                                \
            if (e_ != hipSuccess) return mr_fail((ctx), MR_ERR_HIP, "%s: %s", name, hipGetErrorString(e_)); \
        }                                                                                                  \
    } while (0)

// an A/B and test knob that is on unless set to 0 (read per call: tests flip them)
inline bool knob_on(const char* name) {
    const char* e = getenv(name);
    return !(e && atoi(e) == 0);
}

// ops of the fused kernel's walk: a wide graph's hot ops, else all
inline int32_t kern_n(const mr_graph* g) { return g->wide ? g->NA : g->N; }

// ---------------------------------------------------------------- mr_pagerank.hip
int mr_pagerank_batch_impl(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, double alpha,
                           int iters, int precision, uint32_t flags, bool sharded = false, double* last_resid = nullptr);

// ---------------------------------------------------------------- mr_pr_plan.hip
// k_tr_a's LDS image (TrLds, mr_pr_walk.h) of a graph of N ops: every op's su fits beside the accumulator; the
// hot-op mask sums fit too
bool tr_su_fits(int32_t N);
bool tr_hot_fits(int32_t N);

// ---------------------------------------------------------------- mr_pr_kinds.hip
uint64_t kind_seed(int a);
uint64_t kind_hmask(int a);
int64_t kind_part_min();
int graph_kinds(mr_ctx* ctx, mr_graph* g, bool chk, bool ktab, uint64_t cap, uint64_t seed, uint64_t hmask);
int kind_compressed_call(mr_ctx* ctx, mr_graph* g, int anomaly, double d, double alpha, int iters, int precision,
                         uint32_t flags);

// ---------------------------------------------------------------- mr_pr_setup.hip
// kinds, preference vector and iteration state of one graph (everything before the iterations)
int pagerank_setup(mr_ctx* ctx, mr_graph* g, int anomaly, double d, bool fp32, uint32_t flags, bool sharded,
                   uint64_t seed, uint64_t hmask);
bool setup_batchable(const mr_graph* g, uint32_t flags);
// keep / dkeep: the batched set-up's descriptors (host and device bytes), owned by the caller until
// its stream work is done
int pagerank_setup_batch(mr_ctx* ctx, mr_graph* const* gs, const int* anomaly, int ng, double d, bool fp32,
                         uint64_t seed, uint64_t hmask, std::vector<unsigned char>& keep, DBuf<unsigned char>& dkeep);
// k_inv_perm / k_pr_reset on ctx's stream
void inv_perm_launch(mr_ctx* ctx, const int32_t* perm, int32_t n, int32_t* inv);
void pr_reset_launch(mr_ctx* ctx, int32_t T, int64_t cap, int32_t N, float* pref, float* c_t, unsigned long long* hk,
                     KCnt* cr, int32_t* flag, double* scal);

// ---------------------------------------------------------------- mr_pr_shard.hip
int shard_kinds(mr_ctx* ctx, mr_graph* g, uint64_t cap);
int shard_exchange(mr_ctx* ctx, mr_graph* g);
