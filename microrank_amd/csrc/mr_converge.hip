// Convergence of the power iteration: how far the rank vector moved in one iteration.
//
// The reference runs a fixed 25 iterations (pagerank.py:117) and its README's production notices
// say a large system "needs more iterations in PageRank" (README.md:37); nothing there measures
// whether a count was enough.  k_resid does: after iteration `it` the unnormalised s' sits in
// spb[(it+1)&1] with its maximum in ring slot (it+1)%3, the previous one in spb[it&1] with slot
// it%3 (both valid until the next launch clears slot it%3), so
//   resid(it) = max_o | spb[(it+1)&1][o] / M_s(it+1) - spb[it&1][o] / M_s(it) |
// is the L-infinity distance between the vectors the reference holds in `s` after it+1 and after
// `it` iterations (pagerank.py:126; s_0 is the unnormalised 1/(N+T) of :118, M_s(0) = 1).  A max
// needs no op order: relabelled graphs are read as they lie.  spb is fp64 in both precisions.
//
// A history (mr_pagerank_converge, the window entries' tol form) runs it after every iteration, which
// rules out pf launches.  The report of a fixed count runs it once, after the LAST iteration, in any
// launch form: launch K-1 cleared slot (K+1)%3, a pf launch's block 0 published s_{K-1} and M_s(K-1)
// to spb[(K-1)&1] and slot (K-1)%3 in its prologue, the closing k_fx_b (or the last block's finish)
// wrote spb[K&1] and slot K%3, and nothing runs after them (K = 1: the set-up's s_0, M_s(0) = 1).
#include "mr_iter_dev.h"
#include "mr_prim.h"

constexpr int RESID_T = 256;                     // threads per block
constexpr int RESID_PER = RESID_OPS / RESID_T;   // ops per thread: RESID_PER / 2 16-byte loads per vector
static_assert(RESID_OPS % (2 * RESID_T) == 0, "a block's ops split into double2 per thread");

__global__ void __launch_bounds__(RESID_T) k_resid(const GDev* __restrict__ gs, int32_t ng, int it, int stride, int slot,
                                                   int store, unsigned long long* __restrict__ resid) {
    __shared__ double red[RESID_T / WAVE];
    // the graph owning the block (blk0r is non-decreasing over the graphs; every graph has a block)
    const int32_t gi = block_owner<GDev, &GDev::blk0r>(gs, ng, (int32_t)blockIdx.x);
    const GDev& G = gs[gi];
    const int32_t N = G.N;
    const double* __restrict__ sa = G.spb[(it + 1) & 1];
    const double* __restrict__ sb = G.spb[it & 1];
    // M_s of both iterations: the MSH s-shards of their ring slots, as weights_body reads them
    // (every wave reduces them itself: 64 lanes, 64 shards)
    const int lane = threadIdx.x & (WAVE - 1);
    const double Ma = wave_max(bits2d(G.mslot[(size_t)2 * MSH * ((it + 1) % 3) + lane]));
    const double Mb = wave_max(bits2d(G.mslot[(size_t)2 * MSH * (it % 3) + lane]));
    const int32_t base = ((int32_t)blockIdx.x - G.blk0r) * RESID_OPS;
    double m = 0.0;
    if (base + RESID_OPS <= N) {   // a whole block: 16-byte loads, all in flight before the divisions
        double2 a[RESID_PER / 2], b[RESID_PER / 2];
#pragma unroll
        for (int j = 0; j < RESID_PER / 2; ++j) {
            const int32_t o = base + 2 * (j * RESID_T + (int32_t)threadIdx.x);
            a[j] = *reinterpret_cast<const double2*>(sa + o);
            b[j] = *reinterpret_cast<const double2*>(sb + o);
        }
#pragma unroll
        for (int j = 0; j < RESID_PER / 2; ++j) {
            m = nmax(m, fabs(a[j].x / Ma - b[j].x / Mb));
            m = nmax(m, fabs(a[j].y / Ma - b[j].y / Mb));
        }
    } else {   // the graph's last, ragged block
        for (int32_t o = base + (int32_t)threadIdx.x; o < N; o += RESID_T) m = nmax(m, fabs(sa[o] / Ma - sb[o] / Mb));
    }
    m = block_max(m, red);
    // non-negative doubles (and a NaN, sign cleared by fabs) order as their bit patterns: an
    // integer max, so the word does not depend on the blocks' arrival order
    // store: every graph of the launch is one block, which writes its word (no zeroing before it)
    if (threadIdx.x == 0) {
        if (store) resid[(size_t)gi * stride + slot] = d2bits(m);
        else atomicMax(&resid[(size_t)gi * stride + slot], d2bits(m));
    }
}

void mr_resid_launch(mr_ctx* ctx, const GDev* dv, int ng, int32_t blocks, int it, int stride, int slot, bool store,
                     unsigned long long* resid) {
    hipLaunchKernelGGL(k_resid, dim3(blocks), dim3(RESID_T), 0, ctx->stream, dv, ng, it, stride, slot, store ? 1 : 0, resid);
}
