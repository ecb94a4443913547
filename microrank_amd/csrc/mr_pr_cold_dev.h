// Wide fused graphs (N > FX_NMAX), device side: the cold halves of both products, run per iteration
// before k_tr_a / k_fx_b -- k_cold_trace and k_cold_ops.  Included by mr_pr_tile_cold.hip alone
// (cold_trace_kernel / cold_ops_kernel hand them to iterate).  (WIDE_CT: mr_pr_internal.h)
#pragma once
#include "mr_iter_dev.h"
#include "mr_pr_internal.h"
#include "mr_prim.h"

namespace {

// ---- wide fused graphs, per iteration, before k_tr_a
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

}  // namespace
