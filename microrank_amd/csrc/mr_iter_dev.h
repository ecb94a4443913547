// What the power iteration's kernels share across translation units (the iteration's kernels in
// mr_pr_walk.hip, mr_pr_fxb.hip, mr_pr_tile_cold.hip and mr_pagerank.hip, mr_pr_setup.hip's iteration
// state, mr_converge.hip's residual): the maxima ring, a graph's device descriptor, and the device
// helpers that read the descriptor in more than one of those units.
#pragma once
#include "mr_internal.h"
#include "mr_prim.h"

// M_s / M_r per iteration live in MSH shards (an atomicMax per block or op on ONE word would
// serialise ~2k same-address atomics per iteration); readers reduce the shards.
constexpr int MSH = 64;
// mslot: [3 iterations][s | r][MSH] maxima, then words of the hand-offs (6 MSH + 1: the last-block ticket)
constexpr int MSLOT_WORDS = 6 * MSH + 8;
__device__ __forceinline__ double bits2d(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ unsigned long long d2bits(double v) {
    return (unsigned long long)__double_as_longlong(v);
}

// Per-graph view for the batched iteration: one k_iter_a / k_iter_b pair per Jacobi iteration
// covers every graph of a batch (the two graphs of an RCA window, or many windows); graph i owns
// blocks [blk0, blk0 + n_tb + n_tiles) of k_iter_a and [blk0b, blk0b + n_ob) of k_iter_b.
struct GDev {
    const int64_t* rs_off;
    const int32_t* rs_ops;
    const uint16_t* rs16;       // u16 copy of rs_ops (N <= 65536) or null
    const uint16_t* rsw;        // the fused kernel's ids: rs16, or rsp in relabelled ops
    const int32_t* perm;        // relabelled ops: perm[new] = old (null: identity)
    int32_t n_hot;              // k_tr_a: su of ops [0, n_hot) in LDS (relabelled graphs)
    const uint16_t* tids;       // k_tr_a: lane-interleaved id chunks of the wave tiles
    const int32_t* coff;        // [n_wt+1] first chunk of a tile
    const int32_t* wtile;       // [waves+1] first tile of each wave of the launch
    const float* c_tp;          // c_t, w_t in position order (tperm)
    const float* w_tp;
    const double* mw_tp;        // kind-compressed graphs: w_t * multiplicity (position order), else null
    const uint8_t* hmask;       // register-accumulated hot ops: trace bits in position order (nhr > 0)
    const uint8_t* trun;        // layout-order graphs: run lengths of identical traces by position (or null)
    const uint32_t* ctids;      // wide graphs: cold chunks of the short-tile walk ([chunk][lane] x 2 labels)
    const int32_t* ccoff;       // [n_wt+1] first cold chunk of a tile
    int32_t nhr;
    int32_t hop[8];
    const float* c_t;
    const float* w_t;
    const float* u_o;
    const float* pw;
    const uint16_t* ltr;
    const int64_t* pr_beg;
    const int32_t* tile_pr0;
    const int32_t* lp;
    const int32_t* tile_lp0;
    const int32_t* op_pr_off;
    const int32_t* op_pr;
    const int64_t* ss_off;
    const int32_t* ss_par;
    void* q[2];
    double* sub[2];
    float* suf[2];                 // su32 graphs: the same su as floats (k_tr_a EXT & TR_X_W32 gathers these)
    double* spb[2];
    double* part;
    unsigned long long* mslot;
    double *sn, *weight, *scal;    // k_weights_batch: normalised s, weights, scalars
    const int32_t* flag;           // the graph's error words (gathered after the iterations)
    unsigned long long* fx_part;
    double* fx_ssv;
    unsigned long long* fx_limb;   // sharded: [2N] (lo, hi) limb sums per op, then [nranks] r' maxima
    int32_t rank, nranks;          // sharded: this rank's slot of the r' maxima appended to the sum
    double* op_sum;                // sharded tile path: [N] pair-partial sums per op
    double fx_scale, fx_iscale;
    const double* dscale;          // k_tr_a graphs cut on the device: {2^SC, 2^-SC} (k_tr_cut), else null
    // wide fused graphs: k_tr_a's ops [0, NA) (NA = N otherwise); ops [NA, N) in ranges of
    // cold_rw ops whose rows (cold_part, blocks cold_rowbase[r] .. [r+1]) carry scale cx_scale
    int32_t NA, cold_rw;
    int32_t ns_warm;               // k_tr_a EXT & TR_X_W32: labels [NA, ns_warm) have their su in LDS (else NA)
    int32_t su32;                  // fp32 wide graphs: su rounded to float where k_fx_b makes it
    const double* cold_acc;        // [T] per position: the cold half of the trace's su sum
    const unsigned long long* cold_part;
    const int32_t* cold_rowbase;
    double cx_scale, cx_iscale;
    double alpha;                  // P_ss weight (k_fx_b's call-graph term)
    int32_t T, N, n_tb, n_tiles, tshift, lds_su, blk0, n_ob, blk0b;
    int32_t blk0f, n_fa, blk0fb, n_fb;   // fused path: k_tr_a / k_fx_b block ranges
    int32_t fb_ops;                      // k_fx_b ops per block
    int32_t lastfin;                     // k_tr_a's last block of the graph finishes the iteration (no k_fx_b)
    int32_t pf;                          // k_tr_a(it) first finishes iteration it - 1 itself (no k_fx_b between)
    int64_t pf_stride;                   // pf: words of one partial-row buffer (rows and terms double-buffered)
    int32_t lf_acq;                      // lastfin: the finishing block takes an agent acquire (else the launch
                                         // runs one workgroup per CU and the sc1 hand-off of the guide's row 1 holds)
    int32_t ssv_pre;                     // k_tr_a's blocks compute the call-graph terms (fx_ssv) for k_fx_b
    int32_t row_wt;                      // k_tr_a's partial rows stored write-through (sc1)
    int32_t blk0r;                       // k_resid: the graph's first block (RESID_OPS ops per block)
};

// The convergence residual (mr_converge.hip): after iteration `it` of a launch's ng graphs,
// resid[g * stride + slot] = bits of max_o |spb[(it+1)&1][o] / M_s(it+1) - spb[it&1][o] / M_s(it)|,
// one block per RESID_OPS ops of a graph (GDev::blk0r; `blocks` over the launch).  A history takes
// stride = max_iters, slot = it; a report of the last iteration alone stride 1, slot 0 (one word
// per graph).  The words are zero before the launch (an integer max of non-negative doubles'
// bits: order-free) -- or, store: every graph is one block (blocks == ng), which stores its word.
constexpr int32_t RESID_OPS = 4096;
void mr_resid_launch(mr_ctx* ctx, const GDev* dv, int ng, int32_t blocks, int it, int stride, int slot, bool store,
                     unsigned long long* resid);

// ---------------------------------------------------------------- device helpers of the iteration's kernels
// (internal linkage: each unit that includes them inlines its own copy)
namespace {

// global-memory views of pointers read from GDev: loads through them compile to global_load
// (vmcnt only) instead of flat_load, whose lgkmcnt share would make every LDS wait also wait
// for outstanding HBM loads
#define GLB __attribute__((address_space(1)))
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ __forceinline__ const GLB T* gp(const T* p) { return (const GLB T*)p; }
template <class T>
__device__ __forceinline__ GLB T* gpw(T* p) { return (GLB T*)p; }

// the graph owning a block of a launch: block_owner (mr_prim.h) over the launch's start offset --
// blk0 k_iter_a, blk0b k_iter_b, blk0f k_tr_a, blk0fb k_fx_b -- non-decreasing over graphs (graphs
// without blocks in a launch repeat it)
// graph of a fused-launch block: ng <= 2 resolves from the scalar split (no memory hop)
template <int32_t GDev::*FIRST>
__device__ __forceinline__ int32_t fx_graph(const GDev* gs, int32_t ng, int32_t split) {
    if (ng == 1) return 0;
    if (ng == 2) return (int32_t)blockIdx.x >= split ? 1 : 0;
    return block_owner<GDev, FIRST>(gs, ng, (int32_t)blockIdx.x);
}

// One collective per sharded iteration: the r' maximum of this rank travels with the per-op sums
// in a one-hot slot per rank (its bit pattern, or the double itself in an fp64 sum: x + 0 = x),
// so the SUM all-reduce also delivers every rank's maximum.  put: a wave reduces this rank's MSH
// shards into slot[rank] and zeroes the other slots; take: the max over the slots joins the shards.
template <class W>
__device__ __forceinline__ void rmax_put(const GDev& G, const unsigned long long* Mnext, W* slots, int lane) {
    const double m = wave_max(bits2d(Mnext[MSH + lane]));
    for (int j = lane; j < G.nranks; j += WAVE) {
        if constexpr (sizeof(W) == 8 && (W)0.5 == (W)0) slots[j] = j == G.rank ? (W)d2bits(m) : (W)0;
        else slots[j] = j == G.rank ? (W)m : (W)0;
    }
}
__device__ __forceinline__ void rmax_take_bits(const unsigned long long* slots, int n, unsigned long long* Mnext, int lane) {
    unsigned long long b = 0ull;
    for (int j = lane; j < n; j += WAVE) b = max(b, slots[j]);
    const double m = wave_max(bits2d(b));
    if (lane == 0) atomicMax(&Mnext[MSH], d2bits(m));
}
__device__ __forceinline__ void rmax_take_f64(const double* slots, int n, unsigned long long* Mnext, int lane) {
    double b = 0.0;
    for (int j = lane; j < n; j += WAVE) b = nmax(b, slots[j]);
    const double m = wave_max(b);
    if (lane == 0) atomicMax(&Mnext[MSH], d2bits(m));
}

}  // namespace
