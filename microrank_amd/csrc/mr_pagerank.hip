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
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <queue>
#include <type_traits>

#include "mr_iter_dev.h"
#include "mr_pr_internal.h"
#include "mr_prim.h"
#include "mr_sort.h"

namespace {

constexpr int LDS_NODES = 8192;     // su staged in LDS up to this many nodes (64 KiB)
constexpr int VCAP = 2048;          // trace-role ids staged per round in LDS (16 KiB of values)

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

// ---------------------------------------------------------------- iteration
// (the maxima ring -- MSH, MSLOT_WORDS, bits2d / d2bits -- and GDev: mr_iter_dev.h)
// the graph owning a block of a launch: block_owner (mr_prim.h) over the launch's start offset --
// blk0 k_iter_a, blk0b k_iter_b, blk0f k_tr_a, blk0fb k_fx_b -- non-decreasing over graphs (graphs
// without blocks in a launch repeat it)

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

// trace role inner loop: the block's id range in rounds of VCAP ids, all loads in flight before
// the LDS gathers, then each thread continues its own trace's sum in node order
template <class ID>
__device__ __forceinline__ double trace_sums(const ID* __restrict__ ids, int64_t e0, int64_t e1, int64_t a, int64_t b,
                                             const double* su, double* vals) {
    double acc = 0.0;
    for (int64_t lo = e0; lo < e1; lo += VCAP) {
        const int64_t hi = min(lo + (int64_t)VCAP, e1);
        __syncthreads();
        int32_t id[VCAP / TB];
#pragma unroll
        for (int j = 0; j < VCAP / TB; ++j) id[j] = (int32_t)ids[min(lo + threadIdx.x + (int64_t)j * TB, hi - 1)];
#pragma unroll
        for (int j = 0; j < VCAP / TB; ++j) {
            const int64_t e = lo + threadIdx.x + (int64_t)j * TB;
            if (e < hi) vals[e - lo] = su[id[j]];
        }
        __syncthreads();
        const int64_t x0 = max(a, lo), x1 = min(b, hi);
        int64_t e = x0;
        for (; e + 4 <= x1; e += 4) {
            const double v0 = vals[e - lo], v1 = vals[e + 1 - lo], v2 = vals[e + 2 - lo], v3 = vals[e + 3 - lo];
            acc += v0;
            acc += v1;
            acc += v2;
            acc += v3;
        }
        for (; e < x1; ++e) acc += vals[e - lo];
    }
    return acc;
}

// Iteration k, first half.  Maxima are exchanged as the bit patterns of non-negative doubles
// through atomicMax; slot k%3 holds (M_s(k), M_r(k)), slot (k+1)%3 collects iteration k+1, slot
// (k+2)%3 is cleared here for k+2.  s' is carried unnormalised together with su'[o] = u_o*s'[o];
// the division by M_s(k) is applied to each finished sum instead of to every term.
template <class Q>
__global__ void __launch_bounds__(TB) k_iter_a(const GDev* __restrict__ gs, int32_t ng, double d, int it) {
    extern __shared__ double lds[];
    __shared__ double red[TB / WAVE];
    __shared__ double msr;
    __shared__ int32_t sg;
    if (threadIdx.x == 0) sg = block_owner<GDev, &GDev::blk0>(gs, ng, (int32_t)blockIdx.x);
    __syncthreads();
    const GDev& G = gs[sg];
    const int32_t lb = (int32_t)blockIdx.x - G.blk0;
    const int cur = it & 1, nxt = cur ^ 1, k3 = it % 3;
    const int32_t T = G.T, N = G.N;
    unsigned long long* mslot = G.mslot;
    const unsigned long long* Mcur = mslot + (size_t)2 * MSH * k3;   // [k%3][s|r][MSH]
    unsigned long long* Mnext = mslot + (size_t)2 * MSH * ((k3 + 1) % 3);
    if (lb == 0 && threadIdx.x < 2 * MSH) mslot[(size_t)2 * MSH * ((k3 + 2) % 3) + threadIdx.x] = 0ull;
    if (lb < G.n_tb) {
        // ---- trace role (pagerank.py:125)
        const int32_t t0 = lb * TB;
        const int32_t t1 = min(t0 + TB, T);
        const int32_t t = t0 + threadIdx.x;
        const bool own = t < T;
        const int64_t e0 = G.rs_off[t0], e1 = G.rs_off[t1];
        const int64_t a = own ? G.rs_off[t] : 0, b = own ? G.rs_off[t + 1] : 0;
        const double* su = G.sub[cur];
        if (G.lds_su) {
            for (int32_t o = threadIdx.x; o < N; o += TB) lds[o] = su[o];
            su = lds;
        }
        if (threadIdx.x < WAVE) {
            const double ms = wave_max(bits2d(Mcur[threadIdx.x]));
            if (threadIdx.x == 0) msr = ms;
        }
        double* vals = lds + (G.lds_su ? N : 0);
        const double acc = G.rs16 ? trace_sums(G.rs16, e0, e1, a, b, su, vals) : trace_sums(G.rs_ops, e0, e1, a, b, su, vals);
        __syncthreads();   // msr (also when the block's id range is empty)
        double rmax = -__builtin_huge_val();
        if (own) {
            const double rp = d * (acc / msr) + (double)G.c_t[t];
            ((Q*)G.q[nxt])[t] = (Q)((double)G.w_t[t] * rp);
            rmax = rp;
        }
        rmax = block_max(rmax, red);
        // a block with no trace (an empty shard's placeholder) leaves -inf: no bits to max in
        if (threadIdx.x == 0 && rmax >= 0.0) atomicMax(&Mnext[MSH + blockIdx.x % MSH], d2bits(rmax));
        return;
    }
    // ---- tile role: partial sums of q_k over each (tile, op) pair  (pagerank.py:122-124, P_sr r)
    const int32_t tile = lb - G.n_tb;
    if (tile >= G.n_tiles) return;
    Q* qs = (Q*)lds;
    const Q* __restrict__ qg = (const Q*)G.q[cur];
    const int32_t tb0 = tile << G.tshift;
    const int32_t nt = min(1 << G.tshift, T - tb0);
    const int32_t p0 = G.tile_pr0[tile], p1 = G.tile_pr0[tile + 1];
    const int32_t l0 = G.tile_lp0[tile], l1 = G.tile_lp0[tile + 1];
    for (int32_t i = threadIdx.x; i < nt; i += TB) qs[i] = qg[tb0 + i];
    __syncthreads();
    const uint16_t* __restrict__ ltr = G.ltr;
    const int64_t* __restrict__ pr_beg = G.pr_beg;
    double* part = G.part;
    for (int32_t p = p0 + (int32_t)threadIdx.x; p < p1; p += TB) {   // short pairs: one thread each
        const int64_t b = pr_beg[p], e = pr_beg[p + 1];
        if (e - b > LONG_PAIR) continue;
        double sum = 0.0;
        for (int64_t j = b; j < e; ++j) sum += (double)qs[ltr[j]];
        part[p] = sum;
    }
    const int lane = threadIdx.x & (WAVE - 1);
    for (int32_t i = l0 + (int32_t)(threadIdx.x / WAVE); i < l1; i += TB / WAVE) {   // long pairs: one wave each
        const int32_t p = G.lp[i];
        const int64_t b = pr_beg[p], e = pr_beg[p + 1];
        double sum = 0.0;
        for (int64_t j = b + lane; j < e; j += WAVE) sum += (double)qs[ltr[j]];
        sum = wave_sum(sum);
        if (lane == 0) part[p] = sum;
    }
}

// Iteration k, second half: a wave per op combines the op's pair partials in tile order and adds
// the call-graph term: s'[o] = d * (sum / M_r(k) + alpha * sum_p pw_p s_k[p] / M_s(k))  (:122-124)
// Sharded graphs (traces split over ranks) run it twice around an fp64 SUM all-reduce of the
// per-op sums: mode 1 writes this rank's sum to op_sum, mode 2 finishes from the reduced op_sum.
__global__ void __launch_bounds__(TB) k_iter_b(const GDev* __restrict__ gs, int32_t ng, double d, double alpha, int it,
                                               int mode) {
    __shared__ int32_t sg;
    if (threadIdx.x == 0) sg = block_owner<GDev, &GDev::blk0b>(gs, ng, (int32_t)blockIdx.x);
    __syncthreads();
    const GDev& G = gs[sg];
    const int32_t o = ((int32_t)blockIdx.x - G.blk0b) * (TB / WAVE) + (int32_t)(threadIdx.x / WAVE);
    if (o >= G.N) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int cur = it & 1, nxt = cur ^ 1, k3 = it % 3;
    const unsigned long long* Mcur = G.mslot + (size_t)2 * MSH * k3;
    unsigned long long* Mnext = G.mslot + (size_t)2 * MSH * ((k3 + 1) % 3);
    double sum = 0.0;
    if (mode != 2) {
        for (int32_t i = G.op_pr_off[o] + lane; i < G.op_pr_off[o + 1]; i += WAVE) sum += G.part[G.op_pr[i]];
        sum = wave_sum(sum);
        if (mode == 1) {
            if (lane == 0) G.op_sum[o] = sum;
            if (o == 0) rmax_put(G, Mnext, G.op_sum + G.N, lane);   // this rank's r' max, one-hot
            return;
        }
    } else {
        sum = G.op_sum[o];
        if (o == 0) rmax_take_f64(G.op_sum + G.N, G.nranks, Mnext, lane);
    }
    const double Ms = wave_max(bits2d(Mcur[lane])), Mr = wave_max(bits2d(Mcur[MSH + lane]));
    const double* sp_cur = G.spb[cur];
    double bb = 0.0;
    for (int64_t e = G.ss_off[o] + lane; e < G.ss_off[o + 1]; e += WAVE) {
        const int32_t p = G.ss_par[e];
        bb += (double)G.pw[p] * sp_cur[p];
    }
    bb = wave_sum(bb);
    if (lane == 0) {
        const double v = d * (sum / Mr + alpha * (bb / Ms));      // pagerank.py:122-124
        G.spb[nxt][o] = v;
        G.sub[nxt][o] = (double)G.u_o[o] * v;
        atomicMax(&Mnext[o % MSH], d2bits(v));
    }
}

// ---------------------------------------------------------------- fused single-pass iteration
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
// (FX_NMAX, and HOT_MAX_WIDE of the hot ops below: mr_pr_internal.h -- the prepare reads them too)

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

// graph of a fused-launch block: ng <= 2 resolves from the scalar split (no memory hop)
template <int32_t GDev::*FIRST>
__device__ __forceinline__ int32_t fx_graph(const GDev* gs, int32_t ng, int32_t split) {
    if (ng == 1) return 0;
    if (ng == 2) return (int32_t)blockIdx.x >= split ? 1 : 0;
    return block_owner<GDev, FIRST>(gs, ng, (int32_t)blockIdx.x);
}

// ---------------------------------------------------------------- fused iteration: LDS budget and su modes
constexpr size_t WV_LDS_MAX = 160 * 1024 - 512;
// su modes of k_tr_a: global gathers only / every op's su in LDS / the n_hot most covered ops' su in
// LDS (relabelled graphs, ops [0, n_hot)), the rest gathered
enum { WV_SU_GLOBAL = 0, WV_SU_ALL = 1, WV_SU_HOT = 2 };

// ---------------------------------------------------------------- fused iteration, trace-parallel (k_tr_a)
// The single-pass iteration with lane = trace.  At prepare a graph's traces are sorted by op
// count (tperm: position -> trace) and cut into wave tiles of 64 positions; a tile stores its
// traces' ids lane-interleaved in chunks of 4 (chunk c = 64 lanes x 4 u16: one coalesced 512-B
// load), padded to the tile's longest trace with N + lane (a zero su slot and a dummy
// accumulator per lane, so pads neither branch nor collide), and each trace rotated by
// (lane mod len): a trace's first op is often a root shared by the whole tile, and rotation
// spreads those atomics over the chunk's four instructions and many lanes' addresses.
// Each wave streams a contiguous run of tiles as ONE chunk stream -- ids three chunks ahead,
// the su of cold ops (WV_SU_HOT / GLOBAL) one chunk ahead, a tile's q, (1-d) v and w one tile
// ahead -- with every load unconditional (clamped), so each use waits for exactly its own load.
// Per entry: one su read (LDS, or the prefetched gather), one add into the lane's own trace sum
// (sequential: deterministic), one LDS u64 atomic of the lane's X_t (integers: order-free).  The
// block synchronises only to clear the accumulator and to write its partial row.
struct TrLds {
    size_t su, lacc, hs, sp, total;
    bool su_lds;      // every op's su fits beside the accumulator (interleaved: 16 B per op)
    bool hot_ok;      // WV_SU_ALL: the hot-op mask sums (256 doubles) fit too
    int32_t n_hot;    // WV_SU_HOT: su of ops [0, n_hot) in LDS
    // the accumulator first, then su (8-B strides: a 32-lane read group spreads over 32 bank
    // pairs, a 16-lane atomic group over 16)
    // pf (every op's su in LDS only): s itself beside su (the launch finished the previous iteration)
    // w32 (fp32 wide graphs, k_tr_a EXT & 8): su as 4-B floats -- the hot ops, their 64 pad slots,
    // then n_warm "warm" cold labels (NA + j at slot NA + 64 + j) in the space the floats free
    int32_t n_warm;
    __host__ __device__ TrLds(int32_t N, int mode, bool pf = false, bool w32 = false) {
        const size_t ns = (size_t)N + TR_PAD;
        su_lds = ns * 16 <= WV_LDS_MAX;
        const bool all = mode == WV_SU_ALL && su_lds;
        const size_t accb = (ns * 8 + 15) / 16 * 16;
        n_hot = 0;
        n_warm = 0;
        if (mode == WV_SU_HOT && accb < WV_LDS_MAX)
            n_hot = (int32_t)std::min<size_t>((size_t)N, (WV_LDS_MAX - accb) / 8 / 64 * 64);
        lacc = 0;
        su = accb;
        total = all ? 2 * accb : accb + (size_t)n_hot * 8;
        if (all && w32 && !pf) {   // (the hot-op mask sums keep their 2 KB)
            const size_t fl = (WV_LDS_MAX - accb - 256 * 8 - 16) / 4;
            n_warm = fl > ns ? (int32_t)((fl - ns) / 64 * 64) : 0;
            total = accb + ((ns + (size_t)n_warm) * 4 + 15) / 16 * 16;
        }
        sp = total;
        if (pf && all) total += accb;
        hs = total;
        hot_ok = all && total + 256 * 8 <= WV_LDS_MAX;
        if (hot_ok) total += 256 * 8;
    }
};

// Short tiles (tiles of exactly NC chunks, NC <= 8: traces of <= 32 ops), su in LDS: a tile is ONE register
// set -- its NC id chunks, q, c = (1-d) v, w (EXT & 1: the kind multiplicity's mw instead),
// the cold half of the sums (EXT & 2), and the chunk offsets of the next two tiles -- loaded
// unconditionally (addresses clamped) one whole tile ahead.  The tile loop is unrolled by two so
// the two register sets alternate by renaming: no register with a load in flight is ever copied,
// so the only memory waits are for loads issued a tile earlier (the ring of tr_walk's general
// loop below rotates per chunk and at tile ends has to copy the next tile's q, which made every
// tile end wait for all loads in flight, the ids three chunks ahead included).  Tiles are sorted
// by length, so a wave's run is a sequence of short-tile tiers (NC = 1, 2, .., 8, each a code copy
// with every count static) and a suffix of longer tiles the general loop takes.  Same per-lane sums
// in the same order as the general loop: bitwise equal results.
// su in k_tr_a's LDS: doubles, or 4-B floats on fp32 wide graphs (EXT & 8: every su value of such
// a graph is rounded to float where it is made, so the float copy is exact)
template <class Q, int EXT>
using TrSu = std::conditional_t<((EXT & 8) != 0) && std::is_same<Q, float>::value, float, double>;
template <class Q, int NC, int EXT>
struct TrTile {
    u32x2 id[NC];
    Q q;
    float c;
    float w;
    double mw;     // EXT & 1: w times the kind multiplicity (kind-compressed graphs)
    u32x2 cid[2];  // EXT & 2: the tile's first two cold chunks (wide graphs: 2 cold labels per lane each)
    double xo;     // EXT & 2: k_cold_trace's sum when the tile has more cold chunks (else a dummy)
    int32_t ccw;   // EXT & 2: lane j: ccoff[k + 1 + j] (the next tile's cold chunk range)
    int32_t cw;    // lane j: coff[k + 1 + j] (readlane 0 / 1: the next tile's chunk range)
    uint32_t hm;   // the trace's hot-op bits (nhr > 0)
    uint32_t rl;   // the run of identical traces this lane heads (0: another lane's run; 1: its own)
    uint32_t rln;  // the next tile's rl (a tail loads nothing of its own: its loads need it a tile ahead)
    u32x2 cidn[2]; // EXT & 8: the NEXT tile's first two cold chunks (its gathers go out a tile early)
    float cf[4];   // EXT & 8: this tile's non-warm cold su, gathered while the previous tile walked
    float xw;      // EXT & 8: this tile's warm cold su (LDS), summed at the previous tile's end
};
// the hot ops of a trace: their su first in the lane's sum (the same order in both walks), X into
// the lane's register accumulators (integers: order-free; flushed once per walk)
// The su part is one LDS read of hs[hm] = the sum of the trace's hot su in h order (k_tr_a builds
// the 256 sums per iteration: adding the absent ops' +0.0 would not change a sum, so hs[hm] is the
// lane's own sequential sum over its hot ops).
template <int HN>
struct TrHot {
    int32_t n;
    const double* hs;   // LDS [256]
    unsigned long long acc[HN];
};
// (every one of the HOT_MAX accumulators is updated: ops past nhr are never in a mask, so they
// add 0 -- no per-op condition, no duplicated registers)
template <int HN>
__device__ __forceinline__ double tr_hot_init(TrHot<HN>& H, uint32_t hm, unsigned long long X) {
#pragma unroll
    for (int h = 0; h < HN; ++h) {
        const unsigned long long sel = (unsigned long long)(long long)(((int32_t)(hm << (31 - h))) >> 31);
        H.acc[h] += X & sel;
    }
    return H.hs[hm];
}
// hs[m] for m = tid < 256 (su of every op in LDS; the caller synchronises before and after)
template <class SU>
__device__ __forceinline__ void tr_hot_sums(const GDev& G, const SU* su_l, double* hs, int32_t tid) {
    if (tid < 256) {
        double a = 0.0;
        for (int h = 0; h < G.nhr; ++h)
            if ((tid >> h) & 1) a += su_l[G.hop[h]];
        hs[tid] = a;
    }
}
template <class Q, int NC, int EXT, int HN>
__device__ __forceinline__ int32_t tr_walk_short(const GDev& G, int32_t k, const int32_t ke, int32_t T, int32_t lane,
                                                 int cur, int nxt, double d, double Ms, double xsc, const TrSu<Q, EXT>* su_l,
                                                 unsigned long long* lacc, double& rmax, TrHot<HN>& H, int32_t& c0,
                                                 int32_t& n, int32_t& q0, int32_t& nq) {
    const GLB int32_t* coff = gp(G.coff);
    const GLB Q* qc = gp((const Q*)G.q[cur]);
    GLB Q* qn = gpw((Q*)G.q[nxt]);
    const GLB float* c_tp = gp(G.c_tp);
    const GLB float* w_tp = gp(G.w_tp);
    // EXT: a graph of the launch may carry mw / cold sums; graphs without them load a valid dummy
    // (su[0]) and select the plain value -- unconditional loads, no branches around them
    const GLB double* sug = gp(G.sub[cur]);
    const bool kc = (EXT & 1) && G.mw_tp, cx = (EXT & 2) && G.cold_acc;
    const GLB double* mw_tp = kc ? gp(G.mw_tp) : sug;
    // wide graphs: the cold entries' su gathered here (issued when a tile starts, summed when it
    // ends: a tile of LDS work hides the L2 latency), no cold_acc pass for these tiles
    const GLB u32x2* cids = gp((const u32x2*)G.ctids) + lane;
    const GLB int32_t* ccoff = cx ? gp(G.ccoff) : coff;
    const int32_t ccl = max(__builtin_amdgcn_readfirstlane(ccoff[ke]) - 1, 0);
    const uint32_t cpad = (uint32_t)(G.N + lane);
    // EXT & 8: cold labels below ns_warm ("warm") read their su from LDS slot label + TR_PAD; the
    // other labels from global memory.  Both reads issue for every slot: the LDS one of a non-warm
    // label reads the lane's zero pad slot NA + lane, the global one of a warm label the lane's zero
    // pad N + lane (one coalesced line per wave) -- the sum of the two is the label's su exactly
    constexpr bool W32 = (EXT & 8) != 0;
    const uint32_t nsw = W32 ? (uint32_t)G.ns_warm : 0u, lzero = W32 ? (uint32_t)(G.NA + lane) : 0u;
    const GLB float* sugf = W32 ? gp((const float*)G.suf[cur]) : nullptr;
    const bool hot = H.n > 0;
    const GLB uint8_t* hmk = hot ? gp(G.hmask) : (const GLB uint8_t*)coff;
    // EXT & 4: run-merged graphs (trun).  Without it the run logic is compiled out: every lane walks
    // its own trace (the headline walk)
    constexpr bool RUNS = (EXT & 4) != 0;
    const GLB uint8_t* trn = RUNS ? gp(G.trun) : nullptr;
    const int32_t cl = __builtin_amdgcn_readfirstlane(coff[ke]) - 1;   // the run's last chunk
    // the first tile's chunk ranges: handed over by the previous tier (n >= 0), else loaded
    if (n < 0) {
        const int32_t v = coff[min(k + lane, ke)];
        c0 = __builtin_amdgcn_readfirstlane(v);
        n = __builtin_amdgcn_readlane(v, 1) - c0;
        if constexpr ((EXT & 2) != 0) {
            const int32_t u = ccoff[min(k + lane, ke)];
            q0 = __builtin_amdgcn_readfirstlane(u);
            nq = __builtin_amdgcn_readlane(u, 1) - q0;
        }
    }
    if (n != NC) return k;
    using R = TrTile<Q, NC, EXT>;
    const GLB double* cacc = cx ? gp(G.cold_acc) : sug;
    // run marks of tile kk's lanes (1 on graphs without runs)
    auto rl_of = [&](int32_t kk) -> uint32_t {
        if constexpr (!RUNS) return 1u;
        return trn ? (uint32_t)trn[min(min(kk, ke - 1) * WAVE + lane, T - 1)] : 1u;
    };
    // a run's tail (rl 0) needs none of its own ids, q, c or w -- the head walks for it and its r'
    // comes by shuffle -- so its loads go to one shared word each (one cache line per load, not
    // its own): unconditional loads, no branch
    const GLB u32x2* idb = gp((const u32x2*)G.tids);
    auto load = [&](R& r, int32_t kk, int32_t cc0, int32_t qq0, int32_t nqq, uint32_t rl, int32_t qn1 = 0) {
        const int32_t kq = min(kk, ke - 1);
        const int32_t p = min(kq * WAVE + lane, T - 1);
        const bool hd = !RUNS || rl != 0u;
        const int32_t ph = hd ? p : 0;
#pragma unroll
        for (int j = 0; j < NC; ++j) r.id[j] = idb[hd ? (size_t)min(cc0 + j, cl) * WAVE + lane : 0];
        r.q = qc[ph];
        r.c = c_tp[ph];
        r.w = w_tp[ph];
        if constexpr ((EXT & 1) != 0) r.mw = mw_tp[kc ? p : 0];
        if constexpr ((EXT & 2) != 0) {
            if (cx) {   // (uniform; ctids exists only on wide graphs)
                if constexpr (W32) {   // tile kk + 1's labels (its first cold chunk qn1)
                    r.cidn[0] = cids[(size_t)min(qn1, ccl) * WAVE];
                    r.cidn[1] = cids[(size_t)min(qn1 + 1, ccl) * WAVE];
                } else {
                    r.cid[0] = cids[(size_t)min(qq0, ccl) * WAVE];
                    r.cid[1] = cids[(size_t)min(qq0 + 1, ccl) * WAVE];
                }
            }
            r.xo = cacc[nqq > 2 ? p : 0];   // (unconditional: a branch here costs ~50 VGPRs)
            r.ccw = ccoff[min(kq + 1 + lane, ke)];
        }
        r.cw = coff[min(kq + 1 + lane, ke)];
        r.hm = hot ? hmk[p] : 0u;   // (uniform)
        r.rl = rl;
        r.rln = rl_of(kk + 1);
    };
    // tile kk from r: lane = position kk * 64 + lane
    // EXT & 8: a tile's cold labels (l4: pads past its cold chunk count), their non-warm su gathered
    // into dst.cf (global; warm labels read the lane's zero pad) and their warm su summed into
    // dst.xw (LDS; non-warm labels read the lane's zero pad slot)
    auto labels = [&](const u32x2 (&cid)[2], int32_t nqq, uint32_t (&l4)[4]) {
        l4[0] = nqq > 0 ? cid[0].x : cpad;
        l4[1] = nqq > 0 ? cid[0].y : cpad;
        l4[2] = nqq > 1 ? cid[1].x : cpad;
        l4[3] = nqq > 1 ? cid[1].y : cpad;
    };
    auto gissue = [&](R& dst, const u32x2 (&cid)[2], int32_t nqq) {
        uint32_t l4[4];
        labels(cid, nqq, l4);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst.cf[i] = sugf[l4[i] < nsw ? cpad : l4[i]];
    };
    auto wsum = [&](R& dst, const u32x2 (&cid)[2], int32_t nqq) {
        uint32_t l4[4];
        labels(cid, nqq, l4);
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) a += (float)su_l[l4[i] < nsw ? l4[i] + (uint32_t)TR_PAD : lzero];
        dst.xw = a;
    };
    // W32: nx = the next tile's register set (its gathers issued here from r.cidn, its warm sum at
    // the end), nqn = the next tile's cold chunk count
    auto run = [&](const R& r, int32_t kk, int32_t qq0, int32_t nqq, R* nx = nullptr, int32_t nqn = 0) {
        const int32_t p = kk * WAVE + lane;
        const bool own = p < T;
        double cg[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (W32)
            if (cx) gissue(*nx, r.cidn, nqn);
        if constexpr ((EXT & 2) != 0 && !W32)
            if (cx) {   // the first two cold chunks' su (pads past the tile's chunk count: N + lane, 0)
#ifdef MR_AB_NOGATHER   // (A/B timing builds only: every gather at the lane's pad -- wrong sums)
                const uint32_t z = (r.cid[0].x ^ r.cid[1].y) & 0u;
                cg[0] = sug[cpad + z]; cg[1] = sug[cpad + z]; cg[2] = sug[cpad + z]; cg[3] = sug[cpad + z];
#else
                const uint32_t l4[4] = {nqq > 0 ? r.cid[0].x : cpad, nqq > 0 ? r.cid[0].y : cpad,
                                        nqq > 1 ? r.cid[1].x : cpad, nqq > 1 ? r.cid[1].y : cpad};
#pragma unroll
                for (int i = 0; i < 4; ++i) cg[i] = sug[l4[i]];
#endif
            }
        // a run of rl identical traces (the same ops in the same order, the same q, c and w: the
        // same sum and r') is walked by its head alone: its X times rl into the accumulators (integers:
        // exactly the rl separate adds), its r' broadcast to the run below
        const bool hd = !RUNS || r.rl != 0u;
        const unsigned long long X0 = own && hd ? (unsigned long long)__double2ull_rn((double)r.q * xsc) : 0ull;
        const unsigned long long X = RUNS ? X0 * (unsigned long long)r.rl : X0;
        double acc = H.n ? tr_hot_init(H, r.hm, X) : 0.0;
        if (hd) {
            double sv[2][4];
            auto rd = [&](const u32x2 w, double* s) {
                s[0] = su_l[w.x & 0xffffu];
                s[1] = su_l[w.x >> 16];
                s[2] = su_l[w.y & 0xffffu];
                s[3] = su_l[w.y >> 16];
            };
            rd(r.id[0], sv[0]);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                if (j + 1 < NC) rd(r.id[j + 1], sv[(j + 1) & 1]);
                const u32x2 w = r.id[j];
                atomicAdd(&lacc[(w.x & 0xffffu)], X);
                atomicAdd(&lacc[(w.x >> 16)], X);
                atomicAdd(&lacc[(w.y & 0xffffu)], X);
                atomicAdd(&lacc[(w.y >> 16)], X);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc += sv[j & 1][i];
            }
        }
        double x = 0.0;   // the cold half, sequential in the trace's cold order (k_cold_trace's)
        if constexpr ((EXT & 2) != 0)
            if (cx) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x += W32 ? (double)r.cf[i] : cg[i];
                if constexpr (W32) {
                    x += (double)r.xw;   // (the warm part after the global one: a fixed order)
                    wsum(*nx, r.cidn, nqn);   // the next tile's warm sum (its labels still in r)
                }
                if (nqq > 2) x = r.xo;   // (rare: > 4 cold entries in a trace of the tile: k_cold_trace's sum)
            }
        double rp = d * ((acc + x) / Ms) + (double)r.c;   // pagerank.py:125
        if (RUNS && trn) {   // (uniform) the run's head's r'
            const unsigned long long hb = __ballot(hd) & (lane == WAVE - 1 ? ~0ull : (2ull << lane) - 1ull);
            rp = __shfl(rp, 63 - __builtin_clzll(hb), WAVE);
        }
        if (own) rmax = nmax(rmax, rp);
        const double wq = kc ? r.mw : (double)r.w;
        qn[own && hd ? p : T] = (Q)(wq * rp);   // q[T]: pad slot (a run's tails never read theirs)
    };
    R A, B;
    if constexpr (W32) {
        // the tier's first tile: its cold labels and gathers here (later tiles' go out a tile early),
        // the next tile's cold range from lanes 1 and 2 of the cold offsets
        const int32_t u3 = ccoff[min(k + lane, ke)];
        const int32_t q1 = __builtin_amdgcn_readlane(u3, 1), nq1 = __builtin_amdgcn_readlane(u3, 2) - q1;
        u32x2 c0v[2];
        c0v[0] = cids[(size_t)min(q0, ccl) * WAVE];
        c0v[1] = cids[(size_t)min(q0 + 1, ccl) * WAVE];
        if (cx) {
            gissue(A, c0v, nq);
            wsum(A, c0v, nq);
        }
        load(A, k, c0, q0, nq, rl_of(k), q1);
        int32_t nqA1 = nq1;   // tile k + 1's cold chunk count
        for (;;) {
            const int32_t c0B = __builtin_amdgcn_readfirstlane(A.cw);
            const int32_t nB = __builtin_amdgcn_readlane(A.cw, 1) - c0B;
            const int32_t qB = __builtin_amdgcn_readfirstlane(A.ccw);
            const int32_t nqB = __builtin_amdgcn_readlane(A.ccw, 1) - qB;
            const int32_t qB1 = __builtin_amdgcn_readlane(A.ccw, 1), nqB1 = __builtin_amdgcn_readlane(A.ccw, 2) - qB1;
            load(B, k + 1, c0B, qB, nqB, A.rln, qB1);
            run(A, k, q0, nq, &B, nqA1);
            if (++k == ke || nB != NC) {
                c0 = c0B, n = nB, q0 = qB, nq = nqB;
                break;
            }
            const int32_t c0A = __builtin_amdgcn_readfirstlane(B.cw);
            const int32_t nA2 = __builtin_amdgcn_readlane(B.cw, 1) - c0A;
            const int32_t qA2 = __builtin_amdgcn_readfirstlane(B.ccw);
            const int32_t nqA2 = __builtin_amdgcn_readlane(B.ccw, 1) - qA2;
            const int32_t qA1 = __builtin_amdgcn_readlane(B.ccw, 1);
            nqA1 = __builtin_amdgcn_readlane(B.ccw, 2) - qA1;
            load(A, k + 1, c0A, qA2, nqA2, B.rln, qA1);
            run(B, k, qB, nqB, &A, nqB1);
            if (++k == ke || nA2 != NC) {
                c0 = c0A, n = nA2, q0 = qA2, nq = nqA2;
                break;
            }
            q0 = qA2, nq = nqA2;
        }
        return k;
    }
    load(A, k, c0, q0, nq, rl_of(k));
    int32_t nA = n, qA = q0, nqA = nq;
    for (;;) {
        // B = tile k + 1 (its ranges from A's offsets), then A's tile
        const int32_t c0B = __builtin_amdgcn_readfirstlane(A.cw);
        const int32_t nB = __builtin_amdgcn_readlane(A.cw, 1) - c0B;
        int32_t qB = 0, nqB = 0;
        if constexpr ((EXT & 2) != 0) {
            qB = __builtin_amdgcn_readfirstlane(A.ccw);
            nqB = __builtin_amdgcn_readlane(A.ccw, 1) - qB;
        }
        load(B, k + 1, c0B, qB, nqB, A.rln);
        run(A, k, qA, nqA);
        if (++k == ke || nB != NC) {
            c0 = c0B, n = nB, q0 = qB, nq = nqB;
            break;
        }
        const int32_t c0A = __builtin_amdgcn_readfirstlane(B.cw);
        nA = __builtin_amdgcn_readlane(B.cw, 1) - c0A;
        if constexpr ((EXT & 2) != 0) {
            qA = __builtin_amdgcn_readfirstlane(B.ccw);
            nqA = __builtin_amdgcn_readlane(B.ccw, 1) - qA;
        }
        load(A, k + 1, c0A, qA, nqA, B.rln);
        run(B, k, qB, nqB);
        if (++k == ke || nA != NC) {
            c0 = c0A, n = nA, q0 = qA, nq = nqA;
            break;
        }
    }
    return k;
}

// The wave's walk of k_tr_a over its run of wave tiles: per entry one
// su read, one add into the lane's trace sum, one LDS u64 atomic of X_t; per tile r' of its traces
// and their next q.  Returns the wave's largest r' (-inf when it owns no trace).
template <class Q, int SUM, int NT, int EXT = 0, bool HOTT = false>
__device__ __forceinline__ double tr_walk(const GDev& G, int32_t lb, int cur, int nxt, int32_t N, int32_t NH, double d,
                                          double Ms, double xsc, const TrSu<Q, EXT>* su_l, unsigned long long* lacc,
                                          const double* hs = nullptr) {
    constexpr bool SUL = SUM == WV_SU_ALL, HOT = SUM == WV_SU_HOT;
    constexpr int NW = NT / WAVE;
    const int32_t T = G.T;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const GLB u32x2* ids = gp((const u32x2*)G.tids) + lane;   // chunk c of this lane: ids[c * WAVE]
    const GLB int32_t* coff = gp(G.coff);
    const GLB Q* qc = gp((const Q*)G.q[cur]);
    GLB Q* qn = gpw((Q*)G.q[nxt]);
    const GLB float* c_tp = gp(G.c_tp);
    const GLB float* w_tp = gp(G.w_tp);
    const GLB double* sug = gp(G.sub[cur]);   // ids >= N are pads (su 0)
    // this wave's tiles [k, ke) (a contiguous run: the host cuts them by chunk count)
    const GLB int32_t* wt = gp(G.wtile) + ((size_t)lb * NW + wv);
    int32_t k = __builtin_amdgcn_readfirstlane(wt[0]);
    const int32_t ke = __builtin_amdgcn_readfirstlane(wt[1]);
    double rmax = -__builtin_huge_val();
    constexpr int HN = (EXT & 2) ? HOT_MAX_WIDE : HOT_MAX;
    TrHot<HN> H;
    H.n = SUL && HOTT ? __builtin_amdgcn_readfirstlane(G.nhr) : 0;   // (the host strips only such graphs)
    H.hs = hs;
#pragma unroll
    for (int h = 0; h < HN; ++h) H.acc[h] = 0ull;
    const int32_t k_first = k;
    if constexpr (SUL) {
        // one tier per chunk count (the run's tiles ascend in it): every count static, no branch
        // inside a tile, so each wait is for exactly the LDS reads and loads it consumes
        int32_t tc0 = 0, tn = -1, tq0 = 0, tnq = 0;   // the next tile's ranges, handed from tier to tier
#define TR_TIER(NC_) if (NC_ <= ((EXT & 8) ? TR_TIERS_W32 : NT == 1024 || (EXT & 3) ? TR_TIERS_EXT : MR_TR_TIERS512) && k < ke) k = tr_walk_short<Q, NC_, EXT, HN>(G, k, ke, T, lane, cur, nxt, d, Ms, xsc, su_l, lacc, rmax, H, tc0, tn, tq0, tnq);
        TR_TIER(1) TR_TIER(2) TR_TIER(3) TR_TIER(4) TR_TIER(5) TR_TIER(6) TR_TIER(7) TR_TIER(8)
#undef TR_TIER
    }
    const GLB uint8_t* hmk = gp(G.hmask);
    if (k < ke) {
        auto pos = [&](int32_t kk) { return min(kk * WAVE + lane, T - 1); };
        // cold-op su of a chunk (LDS-resident ops load sug[0]: one line, no traffic; pads read as 0)
        auto gather = [&](const u32x2 w, double* g) {
            const int32_t o[4] = {(int32_t)(w.x & 0xffffu), (int32_t)(w.x >> 16), (int32_t)(w.y & 0xffffu),
                                  (int32_t)(w.y >> 16)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double v = SUL ? 0.0 : sug[HOT && o[j] < NH ? 0 : min(o[j], N - 1)];
                g[j] = o[j] < N ? v : 0.0;
            }
        };
        int32_t c = __builtin_amdgcn_readfirstlane(coff[k]);
        int32_t ce = __builtin_amdgcn_readfirstlane(coff[k + 1]);   // end of tile k
        const int32_t cl = __builtin_amdgcn_readfirstlane(coff[ke]) - 1;   // the run's last chunk
        // tile k's words; tile k + 1's q and end chunk (one tile ahead, clamped into the run).  The
        // end chunk is loaded per lane (lane-varying address: a vector load -- a scalar load would
        // share lgkmcnt with the LDS traffic and force full drains)
        const int32_t kn = min(k + 1, ke - 1);
        // w_t of a position: times the kind's multiplicity on a kind-compressed graph (uniform branch)
        const GLB double* mw_tp = gp(G.mw_tp);
        auto wq = [&](int32_t kk) { return mw_tp ? mw_tp[pos(kk)] : (double)w_tp[pos(kk)]; };
        double q_cur = (double)qc[pos(k)];
        float c_cur = c_tp[pos(k)];
        // wide graphs: the cold half of the trace's sum (k_cold_trace), else 0 (acc + 0 = acc)
        const GLB double* cacc = gp(G.cold_acc);
        double x_cur = cacc ? cacc[pos(k)] : 0.0;
        double w_cur = wq(k);
        double q_nx = (double)qc[pos(kn)];
        int32_t ce_nx = coff[min(kn + 1 + lane, ke)];
        // su of a chunk's ops from LDS (HOT: the hot part; the cold part comes from gather)
        auto lds_su = [&](const u32x2 w, double* sv) {
            const int32_t o[4] = {(int32_t)(w.x & 0xffffu), (int32_t)(w.x >> 16), (int32_t)(w.y & 0xffffu),
                                  (int32_t)(w.y >> 16)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sv[j] = SUL ? su_l[o[j]] : HOT ? su_l[min(o[j], NH - 1)] : 0.0;
            }
        };
        // ids ring (4 chunks: the current one and three ahead), su ping-pong (current, next)
        u32x2 wa = ids[(size_t)c * WAVE];
        u32x2 wb = ids[(size_t)min(c + 1, cl) * WAVE];
        u32x2 wc = ids[(size_t)min(c + 2, cl) * WAVE];
        u32x2 wd;
        double gA[4], gB[4], sA[4], sB[4];
        if (!SUL) gather(wa, gA);
        if (SUL || HOT) lds_su(wa, sA);
        unsigned long long X = k * WAVE + lane < T ? (unsigned long long)__double2ull_rn(q_cur * xsc) : 0ull;
        double acc = H.n ? tr_hot_init(H, hmk[pos(k)], X) : 0.0;
        // One chunk: ids CUR (here), su SC / GC (LDS here, cold gathers in flight); NXT's cold
        // gathers and LDS reads go out before CUR's atomics (their latency, bank conflicts
        // included, overlaps a whole chunk), and the ids three chunks ahead land in LD.  The loop
        // is unrolled 4x so the ring rotates by renaming, not by register moves (a move of an
        // in-flight register would wait for it).
#define TR_STEP(CUR, NXT, LD, GC, SC, GN, SN)                                                              \
        {                                                                                                  \
            LD = ids[(size_t)min(c + 3, cl) * WAVE];                                                       \
            if (!SUL) gather(NXT, GN);                                                                     \
            if (SUL || HOT) lds_su(NXT, SN);                                                               \
            const int32_t o_[4] = {(int32_t)(CUR.x & 0xffffu), (int32_t)(CUR.x >> 16),                     \
                                   (int32_t)(CUR.y & 0xffffu), (int32_t)(CUR.y >> 16)};                    \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) atomicAdd(&lacc[o_[j]], X);                         \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                  \
                acc += SUL ? SC[j] : HOT ? (o_[j] < NH ? SC[j] : GC[j]) : GC[j];                          \
            if (++c == ce) {                                                                               \
                /* tile k done: r' of its traces (pagerank.py:125) and the next q */                      \
                const int32_t p_ = k * WAVE + lane;                                                        \
                const bool own_ = p_ < T;                                                                  \
                const double rp_ = d * ((acc + x_cur) / Ms) + (double)c_cur;                               \
                if (own_) rmax = nmax(rmax, rp_);                                                          \
                qn[own_ ? p_ : T] = (Q)(w_cur * rp_);   /* q[T]: pad slot */                              \
                if (++k == ke) goto tr_done;                                                               \
                ce = __builtin_amdgcn_readfirstlane(ce_nx);                                                \
                q_cur = q_nx;                                                                              \
                const int32_t kk_ = min(k + 1, ke - 1);                                                    \
                c_cur = c_tp[pos(k)];                                                                      \
                x_cur = cacc ? cacc[pos(k)] : 0.0;                                                         \
                w_cur = wq(k);                                                                             \
                q_nx = (double)qc[pos(kk_)];                                                               \
                ce_nx = coff[min(kk_ + 1 + lane, ke)];                                                     \
                X = p_ + WAVE < T ? (unsigned long long)__double2ull_rn(q_cur * xsc) : 0ull;               \
                acc = H.n ? tr_hot_init(H, hmk[pos(k)], X) : 0.0;                                          \
            }                                                                                              \
        }
        for (;;) {
            TR_STEP(wa, wb, wd, gA, sA, gB, sB)
            TR_STEP(wb, wc, wa, gB, sB, gA, sA)
            TR_STEP(wc, wd, wb, gA, sA, gB, sB)
            TR_STEP(wd, wa, wc, gB, sB, gA, sA)
        }
#undef TR_STEP
    tr_done:;
    }
    // the hot ops' accumulators: a wave sum each (integers), one LDS add
    if (k_first < ke)
#pragma unroll
        for (int h = 0; h < HN; ++h)
            if (h < H.n) {
                unsigned long long a = H.acc[h];
#pragma unroll
                for (int m = WAVE / 2; m >= 1; m >>= 1) a += (unsigned long long)__shfl_xor((long long)a, m, WAVE);
                if (lane == 0) atomicAdd(&lacc[G.hop[h]], a);
            }
    return rmax;
}

// The call-graph term alpha (P_ss s_k)[o] / M_s(k) of k_fx_b (pagerank.py:122-124), computed in
// k_tr_a instead: block lb owns the columns [lb N / n_fa, (lb + 1) N / n_fa), and every wave that
// has finished its walk takes chunks of 64 of them (an LDS counter) -- the chains of dependent
// loads (ss_off -> ss_par -> pw, s_k) then run in the slack of the block's slowest wave, not in
// k_fx_b's critical path.  The same arithmetic as k_fx_b (a lane per column of <= 8 parents with
// wave_sum's butterfly value, a wave per column of more): fx_ssv[o], read there bitwise.
// (pf: s_k from the block's LDS copy spl -- this launch computed it -- and the terms into buffer
// it & 1 of fx_ssv, read by the next launch's prologue or the final k_fx_b)
__device__ __forceinline__ void tr_ssv_share(const GDev& G, int32_t lb, int cur, double Ms, int* ctr, int lane,
                                             const double* spl = nullptr, int64_t ssv_off = 0) {
    const int32_t N = G.N;
    const int32_t oa = (int32_t)((int64_t)lb * N / G.n_fa), ob = (int32_t)((int64_t)(lb + 1) * N / G.n_fa);
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(ctr, WAVE);
        c = __builtin_amdgcn_readfirstlane(c);
        if (oa + c >= ob) return;
        const int32_t o = oa + c + lane;
        const bool on = o < ob;
        const int32_t op = on && G.perm ? G.perm[o] : o;
        const GLB int64_t* ss_off = gp(G.ss_off);
        const GLB int32_t* ss_par = gp(G.ss_par);
        const GLB float* pw = gp(G.pw);
        const GLB double* spg = gp(G.spb[cur]);
        auto sp = [&](int32_t p) -> double { return spl ? spl[p] : spg[p]; };
        double ssv = 0.0;
        bool big = false;
        if (on) {
            const int64_t e0 = ss_off[op], e1 = ss_off[op + 1];
            if (e1 - e0 <= 8) {
                int32_t pp[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) pp[k] = e0 + k < e1 ? ss_par[e0 + k] : -1;
                double t[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = pp[k] >= 0 ? (double)pw[pp[k]] * sp(pp[k]) : 0.0;
                const double bb = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
                ssv = G.alpha * (bb / Ms);
            } else {
                big = true;
            }
        }
        for (uint64_t bm = __ballot(big); bm; bm &= bm - 1) {   // (wave-uniform)
            const int j = __ffsll((unsigned long long)bm) - 1;
            const int32_t opj = G.perm ? G.perm[oa + c + j] : oa + c + j;
            const int64_t e0 = ss_off[opj], e1 = ss_off[opj + 1];
            double bb = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += WAVE) {
                const int32_t pp = ss_par[e];
                bb += (double)pw[pp] * sp(pp);
            }
            bb = wave_sum(bb);
            if (lane == j) ssv = G.alpha * (bb / Ms);
        }
        if (on) {
            if (G.lastfin)   // (write-through: the graph's last block reads it with sc1 loads)
                __hip_atomic_store(gpw((unsigned long long*)G.fx_ssv) + o, (unsigned long long)__double_as_longlong(ssv),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                G.fx_ssv[ssv_off + o] = ssv;
        }
    }
}

// The last k_tr_a block of a graph finishes the iteration itself (small graphs: window batches),
// so an iteration is ONE launch instead of k_tr_a + k_fx_b.  Every block writes its partial row
// and its call-graph terms write-through (sc1, hipMalloc'd pool memory), every wave waits for its
// stores (vmcnt(0)), and behind a workgroup barrier one lane takes a ticket from the graph's
// counter (an agent-scope add, returned); the block whose ticket completes the iteration's count is
// the consumer: it reads every row and does k_fx_b's work for every op -- the same exact limb sums,
// the same call-graph term (a lane per op of <= 8 parents, a wave per op of more: wave_sum's
// butterfly) and the same finish: bitwise k_fx_b's results.  Two forms of the hand-off
// (MI355X_MICROARCH.md, inter-workgroup visibility):
//  * a launch of at most one block per CU (<= num_cus blocks, the dynamic LDS padded past half a
//    CU's 160 KB so no two blocks share a CU: single windows) is the hand-off table's row 1 in
//    every cell -- one lane per storing workgroup adds to ONE unsharded counter, the last adder
//    told by the returned value, the other waves behind a barrier it joins, hipMalloc, one
//    workgroup per CU, 8-B sc1 stores and sc1 loads: no acquire (lf_acq 0);
//  * any other launch (batches: several workgroups per CU) takes the guide's general consumer
//    form: ONE agent acquire on the adding lane, its own vmcnt(0) wait, a workgroup barrier, then
//    the loads (lf_acq 1).  Only the finishing block pays it.
template <int NT>
__device__ __forceinline__ void tr_last_finish(const GDev& G, int it, double d, double Ms,
                                            GLB unsigned long long* Mnext) {
    constexpr int NW = NT / WAVE;
    __shared__ int s_last;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave's row stores are out
    __syncthreads();
    if (tid == 0) {
        const unsigned long long t = __hip_atomic_fetch_add(gpw(G.mslot) + 6 * MSH + 1, 1ull, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t + 1 == (unsigned long long)G.n_fa * (unsigned long long)(it + 1);
        if (last && G.lf_acq) {   // consumer: agent acquire (this CU's L1 invalidated), waited before the barrier
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    const int32_t N = G.N, nb = G.n_fa, nxt = (it & 1) ^ 1;
    const GLB unsigned long long* rows = gp((const unsigned long long*)G.fx_part);
    const GLB double* sp_cur = gp(G.spb[it & 1]);
    const GLB int64_t* ss_off = gp(G.ss_off);
    const GLB int32_t* ss_par = gp(G.ss_par);
    const GLB float* pw = gp(G.pw);
    const GLB float* u_o = gp(G.u_o);
    const double iscale = G.dscale ? G.dscale[1] : G.fx_iscale;
    for (int32_t ob = wv * WAVE; ob < N; ob += NW * WAVE) {   // lane = op
        const int32_t o = ob + lane;
        const bool on = o < N;
        unsigned long long lo = 0ull, hi = 0ull;
        // 16 rows per batch, every load in flight before the sums (indices clamped; repeats not added)
        const int32_t oc = on ? o : N - 1;
        for (int32_t b0 = 0; b0 < nb; b0 += 16) {
            unsigned long long v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                v[k] = __hip_atomic_load(rows + (size_t)min(b0 + k, nb - 1) * N + oc, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (b0 + k < nb) {
                    lo += v[k] & 0xffffffffull;
                    hi += v[k] >> 32;
                }
        }
        double ssv = 0.0;
        bool big = false;
        if (on && G.ssv_pre) {   // every block computed its share of the terms (tr_ssv_share): one load
            ssv = __longlong_as_double((long long)__hip_atomic_load(gp((const unsigned long long*)G.fx_ssv) + o,
                                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        } else if (on) {
            const int64_t e0 = ss_off[o], e1 = ss_off[o + 1];
            if (e1 - e0 <= 8) {
                int32_t pp[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) pp[k] = e0 + k < e1 ? ss_par[e0 + k] : -1;
                double t[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = pp[k] >= 0 ? (double)pw[pp[k]] * sp_cur[pp[k]] : 0.0;
                const double bb = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
                ssv = G.alpha * (bb / Ms);
            } else {
                big = true;
            }
        }
        for (uint64_t bm = __ballot(big); bm; bm &= bm - 1) {   // (wave-uniform)
            const int j = __ffsll((unsigned long long)bm) - 1;
            const int32_t oj = ob + j;
            const int64_t e0 = ss_off[oj], e1 = ss_off[oj + 1];
            double bb = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += WAVE) {
                const int32_t pp = ss_par[e];
                bb += (double)pw[pp] * sp_cur[pp];
            }
            bb = wave_sum(bb);
            if (lane == j) ssv = G.alpha * (bb / Ms);
        }
        if (on) {
            const double sum = ((double)hi * 4294967296.0 + (double)lo) * iscale;
            const double v = d * (sum + ssv);   // pagerank.py:122-124
            G.spb[nxt][o] = v;
            G.sub[nxt][o] = (double)u_o[o] * v;
            atomicMax((unsigned long long*)&Mnext[o % MSH], d2bits(v));
        }
    }
}

#ifndef MR_TR_WPE512
#define MR_TR_WPE512 8   // minimum waves per SIMD asked of the plain 512-thread k_tr_a (A/B builds: 1)
#endif
template <class Q, int SUM, int NT, int EXT>
__global__ void __launch_bounds__(NT, NT == 512 && EXT == 0 && SUM != WV_SU_HOT ? MR_TR_WPE512 : 1) k_tr_a(const GDev* __restrict__ gs, int32_t ng, int32_t split, double d,
                                             double alpha, int it, int32_t unused) {
    constexpr bool SUL = SUM == WV_SU_ALL, HOT = SUM == WV_SU_HOT;
    constexpr int NW = NT / WAVE;
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    __shared__ double red[NW];
    __shared__ double msh[2];
    const GDev& G = gs[fx_graph<&GDev::blk0f>(gs, ng, split)];
    const int32_t lb = (int32_t)blockIdx.x - G.blk0f;
    const int cur = it & 1, nxt = cur ^ 1, k3 = it % 3;
    const int32_t N = G.NA;   // (wide graphs: the hot ops)
    const int32_t tid = (int32_t)threadIdx.x;
    // pf (window batches, 512-thread variant): k_fx_b's finish of the previous iteration runs here,
    // in every block of the graph (below), so an iteration is one launch
    const bool pf = NT == 512 && SUL && EXT == 0 && G.pf;
    constexpr bool W32 = (EXT & 8) != 0;   // (fp32 wide graphs: float su, warm labels in LDS)
    using SU = TrSu<Q, EXT>;
    const TrLds L_(N, SUM, pf, W32);
    const int32_t NH = HOT ? G.n_hot : 0;   // <= L_.n_hot (the host sizes both alike), >= 64
    const GLB double* sug = gp(G.sub[cur]);   // ids >= N are pads (su 0)
    SU* su_l = (SU*)(lraw + L_.su);
    double* sp_l = (double*)(lraw + L_.sp);   // (pf) s_it itself, for the call-graph terms
    unsigned long long* lacc = (unsigned long long*)(lraw + L_.lacc);
    GLB unsigned long long* mslot = gpw(G.mslot);
    GLB unsigned long long* Mcur = mslot + (size_t)2 * MSH * k3;
    GLB unsigned long long* Mnext = mslot + (size_t)2 * MSH * ((k3 + 1) % 3);
    if (lb == 0 && tid < 2 * MSH) mslot[(size_t)2 * MSH * ((k3 + 2) % 3) + tid] = 0ull;
    double pf_max = -__builtin_huge_val();
    if (pf && it > 0) {
        // s_it[o] = d (S_o 2^-SC + alpha (P_ss s_{it-1})[o] / M_s(it-1)) from the previous launch's
        // partial rows and call-graph terms (buffers (it - 1) & 1): k_fx_b's exact limb sums and its
        // expression, so bitwise k_fx_b's values; every block of the graph computes all N of them
        // (a few rows each) -- block 0 also publishes s_it and M_s(it) for the final k_fx_b
        const int pb = (it - 1) & 1;
        const GLB unsigned long long* rows = gp((const unsigned long long*)G.fx_part) + (size_t)pb * G.pf_stride;
        const GLB double* ssvp = gp(G.fx_ssv) + (size_t)pb * N;
        const GLB float* u_o = gp(G.u_o);
        const double iscale = G.dscale ? G.dscale[1] : G.fx_iscale;
        const int32_t nb = G.n_fa;
        GLB double* spo = gpw(G.spb[cur]);
        for (int32_t o = tid; o < N + TR_PAD; o += NT) {
            if (o < N) {
                unsigned long long lo = 0ull, hi = 0ull;
                for (int32_t b = 0; b < nb; ++b) {
                    const unsigned long long v = rows[(size_t)b * N + o];
                    lo += v & 0xffffffffull;
                    hi += v >> 32;
                }
                const double sum = ((double)hi * 4294967296.0 + (double)lo) * iscale;
                const double v = d * (sum + ssvp[o]);   // pagerank.py:122-124
                sp_l[o] = v;
                su_l[o] = (double)u_o[o] * v;
                pf_max = nmax(pf_max, v);
                if (lb == 0) {
                    spo[o] = v;
                    atomicMax((unsigned long long*)&Mcur[o % MSH], d2bits(v));
                }
            } else {
                su_l[o] = 0.0;
                sp_l[o] = 0.0;
            }
        }
    } else if (W32) {   // hot ops, 64 zero pads, then the warm labels N .. ns_warm - 1
        const int32_t nw = G.ns_warm - N;
        for (int32_t o = tid; o < N + TR_PAD + nw; o += NT)
            su_l[o] = (SU)(o < N ? sug[o] : o < N + TR_PAD ? 0.0 : sug[o - TR_PAD]);
    } else if (SUL) {
        for (int32_t o = tid; o < N + TR_PAD; o += NT) su_l[o] = o < N ? sug[o] : 0.0;
        if (pf)
            for (int32_t o = tid; o < N + TR_PAD; o += NT) sp_l[o] = o < N ? G.spb[cur][o] : 0.0;
    }
    for (int32_t o = tid; o < N + TR_PAD; o += NT) lacc[o] = 0ull;
    if (HOT)
        for (int32_t o = tid; o < NH; o += NT) su_l[o] = sug[o];
    __shared__ int s_ssv;   // the call-graph term chunks taken (G.ssv_pre)
    if (tid < WAVE) {
        const double ms = wave_max(bits2d(Mcur[tid]));
        const double mr = wave_max(bits2d(Mcur[MSH + tid]));
        if (tid == 0) {
            msh[0] = ms;
            msh[1] = mr;
            s_ssv = 0;
        }
    }
    __syncthreads();   // accumulator and maxima ready
    if (pf && it > 0) {   // M_s(it): the maximum of the s_it just computed (block_max synchronises)
        const double m = block_max(pf_max, red);
        if (tid == 0) msh[0] = m;
        __syncthreads();
    }
    // hot ops (large graphs: the 1024-thread variant only) -- the mask sums of this iteration's su
    constexpr bool HOTT = SUL && NT == 1024;
    double* hs = (double*)(lraw + L_.hs);
    if (HOTT && L_.hot_ok && G.nhr) {
        tr_hot_sums(G, su_l, hs, tid);
        __syncthreads();
    }
    const double xsc = (G.dscale ? G.dscale[0] : G.fx_scale) / msh[1], Ms = msh[0];
    const double rmax_w = tr_walk<Q, SUM, NT, EXT, HOTT>(G, lb, cur, nxt, N, NH, d, Ms, xsc, su_l, lacc, hs);
    // the call-graph terms of this block's share of the columns, by the waves done walking
    if (G.ssv_pre) tr_ssv_share(G, lb, cur, Ms, &s_ssv, tid & (WAVE - 1), pf ? sp_l : nullptr, pf ? (int64_t)cur * N : 0);
    __syncthreads();
    GLB unsigned long long* prow = gpw(G.fx_part) + (pf ? (size_t)cur * G.pf_stride : 0) + (size_t)lb * N;
    if constexpr (NT == 512) {   // (window-graph variant only: the large graphs' kernel stays as it is)
        if (G.lastfin) {
            for (int32_t o = tid; o < N; o += NT)   // write-through: the last block reads them with sc1 loads
                __hip_atomic_store(prow + o, lacc[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double rmax = block_max(rmax_w, red);
            if (tid == 0 && rmax >= 0.0) atomicMax((unsigned long long*)&Mnext[MSH + blockIdx.x % MSH], d2bits(rmax));
            tr_last_finish<NT>(G, it, d, Ms, Mnext);
            return;
        }
    }
    if (G.row_wt)   // write-through (sc1): the boundary to k_fx_b has no dirty lines to write back
        for (int32_t o = tid; o < N; o += NT)
            __hip_atomic_store(prow + o, lacc[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        for (int32_t o = tid; o < N; o += NT) prow[o] = lacc[o];
    const double rmax = block_max(rmax_w, red);
    if (tid == 0 && rmax >= 0.0)   // -inf: a block without traces (an empty shard's placeholder)
        atomicMax((unsigned long long*)&Mnext[MSH + blockIdx.x % MSH], d2bits(rmax));
}

// Column sums of the partial rows: a block per chunk of FB_OPS consecutive ops (lane = op, so
// every row read is one coalesced 512-B segment), its FB_W waves splitting the rows; the waves'
// limb sums meet in LDS (integers: order-free).  mode 0: whole graph; sharded graphs split it
// around the limb all-reduce: mode 1 writes this rank's limbs (lo, hi) per op to fx_limb, mode 2
// finishes from the reduced limbs.
// FB_W waves per block: 16 for graphs with many partial rows (a large graph alone: ~1k rows per
// op), 4 when every graph of the launch has few (batched window graphs: tens of rows) -- the block
// is then latency-bound (ss term, rows, LDS meet: a chain of dependent loads), and 4-wave blocks
// put the whole grid on the chip in one round instead of several.
constexpr int FB_W = 16, FB_W_SMALL = 4, FB_SMALL_ROWS = 256;
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
constexpr int64_t FB_MANY_BLOCKS = 1024;   // 16-op blocks of a launch from which "many" holds
constexpr int64_t LASTFIN_WORDS = 32768;
constexpr int32_t PF_NMAX = 1024;   // pf launches: ops per graph (three N-word LDS arrays per block)
constexpr int64_t PF_ROWS = 32;     // pf launches: partial rows per graph every block of it sums (C3 windows: up to 19)
#ifndef MR_LF_ONE_CU_LDS
#define MR_LF_ONE_CU_LDS (80 * 1024 + 1024)   // (A/B builds: 0 = every last-block launch takes the acquire)
#endif
constexpr size_t LF_ONE_CU_LDS = MR_LF_ONE_CU_LDS;   // > half of a CU's 160 KB: one block per CU   // k_tr_a's last-block finish: partial-row words it reads (256 KB)
// px.peers (sharded graphs on the peer path, one graph per launch): the exchange is fused in --
// mode 1 pushes the block's limbs (and block 0 this rank's r' maximum) into every rank's slot for
// this rank and stores the round number in the block's flag there; mode 2 block b waits for flag
// (src, b) of every source (px.spin; else k_peer_bwait waited before the launch) and sums the R
// slots in rank order.  Bitwise the all-reduce path: the same integers summed.
template <int FB_W>
__global__ void __launch_bounds__(WAVE * FB_W) k_fx_b(const GDev* __restrict__ gs, int32_t ng, int32_t split,
                                                     double d, int it, int mode, const MrPeerX px) {
    __shared__ unsigned long long slo[FB_W * WAVE], shi[FB_W * WAVE];
    __shared__ double lssv[WAVE];
    __shared__ int s_ok;
    const GDev& G = gs[fx_graph<&GDev::blk0fb>(gs, ng, split)];
    const bool pxo = px.peers != nullptr;   // (uniform)
    const GLB unsigned long long* preg = (const GLB unsigned long long*)px.region;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int32_t OPB = G.fb_ops, GR = WAVE / OPB;
    const int32_t ol = lane % OPB, grp = lane / OPB;
    // o: the column (the fused kernel's op label); op: the graph's op (perm: relabelled graphs)
    const int32_t o0 = ((int32_t)blockIdx.x - G.blk0fb) * OPB;
    const int32_t o = o0 + ol;
    const int32_t N = G.N, nb = G.n_fa;
    const bool on = o < N;
    const int k3c = it % 3;
    // the op's rows: k_tr_a's (stride NA), or on a wide graph its cold range's (stride cold_rw).
    // The first batch of 16 rows per lane is issued before the call-graph term below, so the two
    // chains of dependent loads overlap (window graphs: tens of rows, one batch covers them)
    const int32_t stride = FB_W * GR;
    const GLB unsigned long long* col = gp((const unsigned long long*)G.fx_part);
    int32_t nbl = 0;
    size_t rs = 1;
    if (on && mode != 2) {
        if (o < G.NA) {   // (pf graphs: the final iteration's rows, buffer it & 1)
            col = gp((const unsigned long long*)G.fx_part) + (G.pf ? (size_t)(it & 1) * G.pf_stride : 0) + o;
            nbl = nb;
            rs = (size_t)G.NA;
        } else {
            const int32_t oc = o - G.NA, r = oc / G.cold_rw, rb0 = G.cold_rowbase[r];
            nbl = G.cold_rowbase[r + 1] - rb0;
            col = gp(G.cold_part) + (size_t)rb0 * G.cold_rw + (oc - r * G.cold_rw);
            rs = (size_t)G.cold_rw;
        }
    }
    const int32_t rfirst = w * GR + grp;
    unsigned long long v0[16];
    if (nbl > 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) v0[k] = col[(size_t)min(rfirst + k * stride, nbl - 1) * rs];
    }
    // the call-graph term alpha (P_ss s_k)[op] / M_s(k) (pagerank.py:122-124) of the block's ops: a
    // wave per op, its lanes striding the op's parents, one fixed-order wave sum (a hub op with
    // thousands of parents costs one wave, not one thread).  (Not in mode 1: its sums only.)
    // ssv_pre: k_tr_a computed them (tr_ssv_share) -- one coalesced load
    if (mode != 1 && G.ssv_pre) {
        if (threadIdx.x < (unsigned)OPB)
            lssv[threadIdx.x] = o0 + (int32_t)threadIdx.x < N ? G.fx_ssv[(G.pf ? (size_t)(it & 1) * N : 0) + o0 + threadIdx.x] : 0.0;
    } else if (mode != 1) {
        const double Ms = wave_max(bits2d(G.mslot[(size_t)2 * MSH * k3c + lane]));
        const GLB double* sp_cur = gp(G.spb[it & 1]);
        const GLB int64_t* ss_off = gp(G.ss_off);
        const GLB int32_t* ss_par = gp(G.ss_par);
        const GLB float* pw = gp(G.pw);
        // the wave's ops j = w, w + FB_W, ..: one lane each for ops of <= 8 parents -- the lane
        // forms the wave sum's value itself (the butterfly of wave_sum over 64 slots with the
        // terms in slots 0..7 and zeros elsewhere: adding +0.0 is exact, so only the pairs
        // (l, l+4), (l, l+2), (0, 1) round) -- all the wave's ops in one chain of loads instead
        // of one chain per op; ops with more parents take the wave path after them
        const int32_t nj = (OPB - w + FB_W - 1) / FB_W;
        bool big = false;
        if (lane < nj) {
            const int32_t j = w + lane * FB_W, oj = o0 + j;
            if (oj < N) {
                const int32_t opj = G.perm ? G.perm[oj] : oj;
                const int64_t e0 = ss_off[opj], e1 = ss_off[opj + 1];
                if (e1 - e0 <= 8) {
                    int32_t pp[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) pp[k] = e0 + k < e1 ? ss_par[e0 + k] : -1;
                    double t[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) t[k] = pp[k] >= 0 ? (double)pw[pp[k]] * sp_cur[pp[k]] : 0.0;
                    const double bb = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
                    lssv[j] = G.alpha * (bb / Ms);
                } else {
                    big = true;
                }
            }
        }
        for (uint64_t bm = __ballot(big); bm; bm &= bm - 1) {   // (wave-uniform)
            const int32_t j = w + (int32_t)(__ffsll((unsigned long long)bm) - 1) * FB_W, oj = o0 + j;
            const int32_t opj = G.perm ? G.perm[oj] : oj;
            const int64_t e0 = ss_off[opj], e1 = ss_off[opj + 1];
            double bb = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += WAVE) {
                const int32_t pp = ss_par[e];
                bb += (double)pw[pp] * sp_cur[pp];
            }
            bb = wave_sum(bb);
            if (lane == 0) lssv[j] = G.alpha * (bb / Ms);
        }
    }
    // the finishing lanes' operands, loaded before the rows so both latencies overlap
    const bool fin = w == 0 && lane < OPB && on;
    const int32_t op = fin && G.perm ? G.perm[o] : o;
    const float uo = fin ? G.u_o[op] : 0.0f;
    const int32_t bidx = (int32_t)blockIdx.x - G.blk0fb;
    const size_t par = (size_t)(px.seq & 1) * (size_t)px.R;   // this round's slots: [par + src] x W words
    if (bidx == 0 && w == 1 && mode) {   // r' maxima riding on the limb sum
        unsigned long long* Mn = G.mslot + (size_t)2 * MSH * ((it % 3 + 1) % 3);
        if (!pxo) {
            if (mode == 1) rmax_put(G, Mn, G.fx_limb + 2 * (size_t)N, lane);
            else rmax_take_bits(G.fx_limb + 2 * (size_t)N, G.nranks, Mn, lane);
        } else if (mode == 1) {   // this rank's maximum into word 2N + rank of its slot on every rank
            const double m = wave_max(bits2d(Mn[MSH + lane]));
            if (lane < px.R)
                __hip_atomic_store((GLB unsigned long long*)px.peers[lane] + px.slots + (par + px.rank) * px.W +
                                       2 * (size_t)N + px.rank,
                                   d2bits(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (pxo && mode == 2) {
        if (px.spin && threadIdx.x == 0) {   // flag (src, bidx) of every source: this round's words are in
            s_ok = 1;
            const unsigned long long need = px.seq + 1, t0 = __builtin_amdgcn_s_memrealtime();
            for (int r = 0; r < px.R && s_ok; ++r)
                while (__hip_atomic_load(preg + px.bflags + (int64_t)r * px.nbf + bidx, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM) < need) {
                    __builtin_amdgcn_s_sleep(2);
                    // a round that already timed out (this call's error word): stop at once instead
                    // of spinning the full timeout again in every later iteration
                    if (__builtin_amdgcn_s_memrealtime() - t0 > px.timeout ||
                        __hip_atomic_load(preg + px.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ull) {
                        s_ok = 0;
                        __hip_atomic_store((GLB unsigned long long*)px.region + px.err, 1ull, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
        } else if (!px.spin && threadIdx.x == 0) {
            s_ok = 1;
        }
        __syncthreads();
        if (!s_ok) return;   // (the error word reports it; the host raises MR_ERR_COMM)
        if (bidx == 0 && w == 1) {   // every rank's r' maximum: word 2N + src of slot src
            unsigned long long b = 0ull;
            for (int j = lane; j < px.R; j += WAVE)
                b = max(b, __hip_atomic_load(preg + px.slots + (par + j) * px.W + 2 * (size_t)N + j, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM));
            const double m = wave_max(bits2d(b));
            if (lane == 0) atomicMax(&G.mslot[(size_t)2 * MSH * ((it % 3 + 1) % 3) + MSH], d2bits(m));
        }
    }
    unsigned long long lo = 0ull, hi = 0ull;
    if (nbl > 0) {
        // the first batch (loaded above), then batches of 16 rows per lane, every load in flight
        // before the sums (indices clamped: the repeats are cache hits and are not added)
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (rfirst + k * stride < nbl) {
                lo += v0[k] & 0xffffffffull;
                hi += v0[k] >> 32;
            }
        for (int32_t r0 = rfirst + 16 * stride; r0 < nbl; r0 += 16 * stride) {
            unsigned long long v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = col[(size_t)min(r0 + k * stride, nbl - 1) * rs];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (r0 + k * stride < nbl) {
                    lo += v[k] & 0xffffffffull;
                    hi += v[k] >> 32;
                }
        }
    }
    // the wave's row groups of one op meet by lane shuffles, the waves through LDS (integers:
    // order-free)
    for (int m = WAVE / 2; m >= OPB; m >>= 1) {
        lo += (unsigned long long)__shfl_xor((long long)lo, m);
        hi += (unsigned long long)__shfl_xor((long long)hi, m);
    }
    if (lane < OPB) {
        slo[w * WAVE + lane] = lo;
        shi[w * WAVE + lane] = hi;
    }
    __syncthreads();
    if (pxo && mode == 1) {   // push the block's limbs to every rank, then the block's flag there
        if (fin) {
            lo = hi = 0ull;
            for (int k = 0; k < FB_W; ++k) {
                lo += slo[k * WAVE + lane];
                hi += shi[k * WAVE + lane];
            }
            for (int r = 0; r < px.R; ++r) {
                GLB unsigned long long* dst = (GLB unsigned long long*)px.peers[r] + px.slots + (par + px.rank) * px.W;
                __hip_atomic_store(dst + 2 * op, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(dst + 2 * op + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (every wave: the r' word of wave 1 too)
        __syncthreads();
        if ((int32_t)threadIdx.x < px.R && !px.mute) {
            __atomic_thread_fence(__ATOMIC_RELEASE);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store((GLB unsigned long long*)px.peers[threadIdx.x] + px.bflags + (int64_t)px.rank * px.nbf + bidx,
                               (unsigned long long)(px.seq + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (!fin) return;
    lo = hi = 0ull;
    for (int k = 0; k < FB_W; ++k) {
        lo += slo[k * WAVE + lane];
        hi += shi[k * WAVE + lane];
    }
    if (mode == 1) {
        G.fx_limb[2 * op] = lo;
        G.fx_limb[2 * op + 1] = hi;
        return;
    }
    if (mode == 2 && pxo) {   // the R slots in rank order (integers: the all-reduce's sum)
        lo = hi = 0ull;
        for (int r = 0; r < px.R; ++r) {
            const GLB unsigned long long* sl = preg + px.slots + (par + r) * px.W;
            lo += __hip_atomic_load(sl + 2 * op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            hi += __hip_atomic_load(sl + 2 * op + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else if (mode == 2) {
        lo = G.fx_limb[2 * op];
        hi = G.fx_limb[2 * op + 1];
    }
    const int nxt = (it & 1) ^ 1, k3 = it % 3;
    unsigned long long* Mnext = G.mslot + (size_t)2 * MSH * ((k3 + 1) % 3);
    const double ssv = lssv[lane];   // (written before the barrier above)
    // hi, lo < 2^53 (fewer than 2^21 rows over all ranks): both conversions exact, one rounding
    const double sum = ((double)hi * 4294967296.0 + (double)lo) * (o < G.NA ? (G.dscale ? G.dscale[1] : G.fx_iscale) : G.cx_iscale);
    const double v = d * (sum + ssv);      // pagerank.py:122-124
    G.spb[nxt][op] = v;
    const double su = (double)uo * v;
    if (G.su32) {   // (fp32 wide graphs: rounded to float, kept both ways)
        const float f = (float)su;
        G.sub[nxt][o] = (double)f;
        G.suf[nxt][o] = f;
    } else {
        G.sub[nxt][o] = su;   // su in the kernel's labels
    }
    atomicMax(&Mnext[op % MSH], d2bits(v));
}

// ---- wide fused graphs, per iteration, before k_tr_a
constexpr int WIDE_CT = 1024;           // k_cold_ops block size
// cold half of each trace's su sum (pagerank.py:125), in position order: k_tr_a adds it to the
// lane's hot sum before the division by M_s(k)
// (over the listed wave tiles only: the long tiles of the general walk and the short tiles with
// more than two cold chunks -- the short-tile walk gathers the rest itself; tiles == nullptr: over
// all ntl wave tiles, for a launch whose k_tr_a has no short-tile walk)
__global__ void k_cold_trace(const int32_t* __restrict__ coff, const int32_t* __restrict__ cops,
                             const double* __restrict__ su, const int32_t* __restrict__ tiles, int32_t ntl, int32_t T,
                             double* __restrict__ cacc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)ntl * WAVE) return;
    const int32_t p = (tiles ? tiles[i / WAVE] : (int32_t)(i / WAVE)) * WAVE + (int32_t)(i % WAVE);
    if (p >= T) return;
    const int32_t a = coff[p], b = coff[p + 1];
    double acc = 0.0;
    int32_t j = a;
    for (; j + 4 <= b; j += 4) {
        const int32_t o0 = cops[j], o1 = cops[j + 1], o2 = cops[j + 2], o3 = cops[j + 3];
        const double v0 = su[o0], v1 = su[o1], v2 = su[o2], v3 = su[o3];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
    }
    for (; j < b; ++j) acc += su[cops[j]];
    cacc[p] = acc;
}
// cold half of P_sr r (pagerank.py:122-124): a block per slice of one range's (position, op)
// pairs, X = rint(q_k[p] / M_r(k) * 2^SCc) added into the range's LDS accumulator; the block's row
// goes out whole (k_fx_b sums a range's rows like k_tr_a's).  SCc leaves no overflow: an op gets
// at most one add per position of the slice (SCc = 64 - bits(widest slice span)).
template <class Q>
__global__ void __launch_bounds__(WIDE_CT) k_cold_ops(const int64_t* __restrict__ cb_beg, const int32_t* __restrict__ cp_pos,
                                                     const uint16_t* __restrict__ cp_op, const void* qv,
                                                     const unsigned long long* mslot, int it, double cx_scale,
                                                     int32_t RW, unsigned long long* __restrict__ cold_part) {
    extern __shared__ unsigned long long cacc_l[];
    __shared__ double mr;
    const Q* __restrict__ q = (const Q*)qv;
    const int k3 = it % 3;
    for (int32_t i = threadIdx.x; i < RW; i += WIDE_CT) cacc_l[i] = 0ull;
    if (threadIdx.x < WAVE) {
        const double m = wave_max(bits2d(mslot[(size_t)2 * MSH * k3 + MSH + threadIdx.x]));
        if (threadIdx.x == 0) mr = m;
    }
    __syncthreads();
    const double xsc = cx_scale / mr;
    const int64_t b = cb_beg[blockIdx.x], e = cb_beg[blockIdx.x + 1];
    int64_t i = b + threadIdx.x;
    for (; i + 3 * WIDE_CT < e; i += 4 * WIDE_CT) {   // four pairs in flight per thread
        int32_t p[4];
        uint16_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[j] = cp_pos[i + j * WIDE_CT];
            o[j] = cp_op[i + j * WIDE_CT];
        }
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (double)q[p[j]];
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&cacc_l[o[j]], (unsigned long long)__double2ull_rn(v[j] * xsc));
    }
    for (; i < e; i += WIDE_CT) atomicAdd(&cacc_l[cp_op[i]], (unsigned long long)__double2ull_rn((double)q[cp_pos[i]] * xsc));
    __syncthreads();
    unsigned long long* row = cold_part + (size_t)blockIdx.x * RW;
    for (int32_t o = threadIdx.x; o < RW; o += WIDE_CT) row[o] = cacc_l[o];
}

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

using TrA = void (*)(const GDev*, int32_t, int32_t, double, double, int, int32_t);
// ext: some graph of the launch carries kind multiplicities (bit 0: mw_tp) or a cold side (bit 1:
// wide graphs) -- only the short-tile walk of the su-in-LDS mode distinguishes them
static TrA tr_kernel(bool fp32, int mode, int NT, int ext = 0) {
    static const TrA tab[2][3][2] = {
        {{k_tr_a<double, 0, 512, 0>, k_tr_a<double, 0, 1024, 0>},
         {k_tr_a<double, 1, 512, 0>, k_tr_a<double, 1, 1024, 0>},
         {k_tr_a<double, 2, 512, 0>, k_tr_a<double, 2, 1024, 0>}},
        {{k_tr_a<float, 0, 512, 0>, k_tr_a<float, 0, 1024, 0>},
         {k_tr_a<float, 1, 512, 0>, k_tr_a<float, 1, 1024, 0>},
         {k_tr_a<float, 2, 512, 0>, k_tr_a<float, 2, 1024, 0>}}};
    static const TrA tab_ext[4][2][2] = {
        {{k_tr_a<double, 1, 512, 1>, k_tr_a<double, 1, 1024, 1>}, {k_tr_a<float, 1, 512, 1>, k_tr_a<float, 1, 1024, 1>}},
        {{k_tr_a<double, 1, 512, 2>, k_tr_a<double, 1, 1024, 2>}, {k_tr_a<float, 1, 512, 2>, k_tr_a<float, 1, 1024, 2>}},
        {{k_tr_a<double, 1, 512, 3>, k_tr_a<double, 1, 1024, 3>}, {k_tr_a<float, 1, 512, 3>, k_tr_a<float, 1, 1024, 3>}},
        {{k_tr_a<double, 1, 512, 4>, k_tr_a<double, 1, 1024, 4>}, {k_tr_a<float, 1, 512, 4>, k_tr_a<float, 1, 1024, 4>}}};
    // ext 10: fp32 wide graphs with float su and warm labels in LDS
    if (ext == 10 && fp32 && mode == WV_SU_ALL) return NT == 1024 ? k_tr_a<float, 1, 1024, 10> : k_tr_a<float, 1, 512, 10>;
    // ext 4: run-merged window graphs (trun; never beside multiplicities or cold sums)
    if (ext == 4 && mode == WV_SU_ALL) return tab_ext[3][fp32 ? 1 : 0][NT == 1024 ? 1 : 0];
    if ((ext & 3) && mode == WV_SU_ALL) return tab_ext[(ext & 3) - 1][fp32 ? 1 : 0][NT == 1024 ? 1 : 0];
    return tab[fp32 ? 1 : 0][mode][NT == 1024 ? 1 : 0];
}

// Launch plan of the fused iteration (k_tr_a) for a batch of graphs (one kernel variant per launch).
struct FxPlan {
    int NT = 1024;      // block size (16 waves; 512 when the graphs are small)
    int mode = WV_SU_ALL;   // su in LDS for every fused graph of the batch / hot ops / none
    bool sul = true;    // mode == WV_SU_ALL
    bool pf = false;    // window batches: the next launch finishes an iteration (k_tr_a's pf prologue)
    bool w32 = false;   // fp32 wide graphs only: float su and warm labels in LDS (k_tr_a EXT & 8)
};
// allow_pf false: k_fx_b every iteration, as under MR_TR_PF=0 (a call that reads the ring between launches)
static FxPlan fx_plan(mr_graph* const* gs, int ng, bool fp32, bool sharded, bool allow_pf = true) {
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
    // ("warm") labels' su, so their cold entries read LDS instead of L2 (k_tr_a EXT & 8);
    // every fused graph of the launch wide and plain (no multiplicities)
#ifndef MR_AB_NO_W32
    P.w32 = fp32 && P.mode == WV_SU_ALL && !P.pf;
#endif
    bool anyf = false;
    for (int i = 0; i < ng && P.w32; ++i)
        if (gs[i]->fused) {
            anyf = true;
            P.w32 = gs[i]->wide && !gs[i]->mw_tp.p && !gs[i]->trun.p;
        }
    P.w32 = P.w32 && anyf;
    return P;
}
static int32_t plan_n_hot(int32_t N, const FxPlan& P) {
    return P.mode == WV_SU_HOT ? TrLds(N, WV_SU_HOT).n_hot : 0;
}
static size_t plan_lds(int32_t N, const FxPlan& P) { return TrLds(N, P.mode, P.pf, P.w32).total; }
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
static int32_t tr_scfix(const mr_graph* g) {
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
#ifdef MR_AB_RFRAC   // (A/B builds: a fraction of the resident slots, leaving room for the builds' blocks)
    R = std::max<int64_t>(1, (int64_t)((double)R * MR_AB_RFRAC));
#endif
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

// algorithmic bytes of one iteration of one graph: op ids once, offsets, the
// r/v/len_t streams, call edges and three N-vectors; o = 4-byte offsets below 2^31 nonzeros
static double iter_bytes(const mr_graph* g, bool fp32) {
    const double w = fp32 ? 4.0 : 8.0, o = g->nnz_sr < (1ll << 31) ? 4.0 : 8.0;
    return 4.0 * (double)g->nnz_sr + o * ((double)g->T + 1) + 4.0 * w * (double)g->T + (8.0 + w) * (double)g->E +
           3.0 * w * (double)g->N;
}

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

// The k_tr_a blocks of every graph (nfa[i]; 0 for a graph off the fused path): ONE tr_split per fused
// graph, its partial rows allocated, and the launch's per-wave cuts in batches (k_tr_cut_b).
static int cut_blocks(mr_ctx* ctx, mr_graph* const* gs, int ng, const FxPlan& plan, HostMarks& hm,
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

// The launch-form knobs (A/B and tests, read once per attempt), each on unless set to 0
struct TrKnobs {
    bool lastfin = knob_on("MR_TR_LASTFIN");   // 0: k_fx_b for every graph
    bool ssv = knob_on("MR_TR_SSV");           // 0: k_fx_b computes the call-graph terms
    bool lfssv = knob_on("MR_TR_LFSSV");       // 0: last-block graphs read the terms through the chain
    // 0: plain partial-row stores.  Write-through measured C4 rank 0 of 8: 43.1 vs 44.6 us per
    // iteration, C4 whole: within noise (two repeats each)
    bool row_wt = knob_on("MR_TR_ROW_WT");
};

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

// A graph's descriptor, part 1: its arrays and sizes, field for field
static void gdev_pointers(GDev& v, const mr_ctx* ctx, const mr_graph* g, bool fp32, double alpha, const FxPlan& plan) {
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
static void gdev_scales(GDev& v, const mr_graph* g, bool sharded, uint64_t cold_span_all) {
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
static void gdev_launch(GDev& v, const mr_graph* g, int64_t nfa, bool fp32, bool sharded, const FxPlan& plan,
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
static int finalise_launch(mr_ctx* ctx, mr_graph* const* gs, int ng, bool fp32, bool sharded, const FxPlan& plan,
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
    int any_ext = 0;   // kind multiplicities (1), cold sums (2) or merged runs (4) in some fused graph of the launch
    for (int i = 0; i < ng; ++i)
        if (gs[i]->fused)
            any_ext |= (hv[(size_t)i].mw_tp ? 1 : 0) | (hv[(size_t)i].cold_acc ? 2 : 0) | (hv[(size_t)i].trun ? 4 : 0);
    if ((any_ext & 4) && (any_ext & 3)) any_ext &= 3;   // (not built: such a launch walks every trace)
    for (int i = 0; i < ng; ++i)   // the wide variant carries HOT_MAX_WIDE hot accumulators
        if ((any_ext & 2) && gs[i]->fused && gs[i]->nhr > HOT_MAX_WIDE)
            return mr_fail(ctx, MR_ERR_ARG, "pagerank batch: a hot-op layout of %d ops beside a wide graph", gs[i]->nhr);
    L.launch_pf = plan.pf;
    for (int i = 0; i < ng; ++i) L.launch_pf = L.launch_pf && (hv[(size_t)i].lastfin || hv[(size_t)i].pf);
    L.launch_pf = L.launch_pf && any_ext == 0;
    if (!L.launch_pf)
        for (int i = 0; i < ng; ++i) {
            if (hv[(size_t)i].pf) hv[(size_t)i].ssv_pre = kn.ssv && !gs[i]->wide && gs[i]->N >= 2048;
            hv[(size_t)i].pf = 0;
        }
    L.tr_a = tr_kernel(fp32, plan.mode, plan.NT, any_ext == 2 && plan.w32 ? 10 : any_ext);
    // a wide graph beside a narrow one whose su does not fit in LDS: the launch leaves WV_SU_ALL, and
    // the kernels of the other modes have no short-tile walk (tr_kernel: no EXT variant), so none of
    // the wide graph's tiles gathers its own cold su -- the general walk reads cold_acc for every
    // tile, and k_cold_trace must then have summed every tile, not only the listed ones
    L.cold_all = (any_ext & 2) && plan.mode != WV_SU_ALL;
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
static int prepare_exchange(mr_ctx* ctx, mr_graph* const* gs, int ng, Launch& L) {
    // wide graphs: k_cold_ops (LDS-bound) runs on the side stream beside k_cold_trace (L2-gather
    // bound) and k_tr_a on the main stream; k_fx_b waits for both
    L.sst = ctx->stream;
#ifndef MR_AB_WIDE_SERIAL   // (A/B builds: k_cold_ops on the main stream)
    if (L.any_wide) {
        if (!ctx->side) {
            MR_TRY_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            for (hipEvent_t& e : ctx->side_ev) MR_TRY_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        L.sst = ctx->side;
    }
#endif
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

// The power iteration: per iteration the wide graphs' cold halves, k_tr_a + k_fx_b for the fused graphs
// and k_iter_a + k_iter_b for the others, a sharded graph's all-reduce between each pair's halves
// Iterations [it_begin, it_end) of the call; cv: the residual of each goes to its history (k_resid,
// outside the roofline bracket)
static int iterate(mr_ctx* ctx, mr_graph* const* gs, int ng, bool fp32, double d, double alpha, int it_begin, int it_end,
                   const FxPlan& plan, const std::vector<GDev>& hv, const GDev* dv, Launch& L,
                   const Converge* cv = nullptr) {
    hipStream_t st = ctx->stream, sst = L.sst;
    const bool side = L.any_wide && sst != st;
    const auto cold_ops = fp32 ? k_cold_ops<float> : k_cold_ops<double>;
    const auto iter_a = fp32 ? k_iter_a<float> : k_iter_a<double>;
    const auto fx_b_k = L.fb_small ? k_fx_b<FB_W_SMALL> : k_fx_b<FB_W>;
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
                hipLaunchKernelGGL(k_cold_trace, dim3(cdiv((int64_t)ntl * WAVE, 256)), dim3(256), 0, st,
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
                hipLaunchKernelGGL(k_iter_b, dim3(L.blocks_b), dim3(TB), 0, st, dv, ng, d, alpha, it, 0);
            } else {   // ONE all-reduce: the per-op P_sr r sums (fp64 SUM) and every rank's r' max
                hipLaunchKernelGGL(k_iter_b, dim3(L.blocks_b), dim3(TB), 0, st, dv, ng, d, alpha, it, 1);
                const int64_t nw = (int64_t)gs[0]->N + ctx->nranks;
                const int prc = mr_peer_allreduce_f64(ctx, gs[0]->op_sum.p, nw);
                if (prc == MR_ERR_STATE) MR_TRY(mr_coll_allreduce(ctx, gs[0]->op_sum.p, nw, MR_DT_F64, 0));
                else MR_TRY(prc);
                hipLaunchKernelGGL(k_iter_b, dim3(L.blocks_b), dim3(TB), 0, st, dv, ng, d, alpha, it, 2);
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
