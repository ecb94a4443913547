// The tile path, device side: the two-launch iteration of general graphs (P_rs != P_sr, pr subsets,
// N > FX_NMAX off the wide path) -- k_iter_a (trace role and tile role; trace_sums its inner loop)
// and k_iter_b.  Included by mr_pr_tile_cold.hip alone (iter_a_kernel / iter_b_kernel hand them to
// iterate); the two-launch scheme itself is described at the top of mr_pagerank.hip.
#pragma once
#include "mr_iter_dev.h"
#include "mr_pr_internal.h"
#include "mr_prim.h"

namespace {

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

}  // namespace
