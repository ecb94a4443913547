// Order statistics from sorted packed keys, shared by mr_slo_quantiles (mr_quantile.hip) and the
// latency evidence (mr_latency.hip): keys (group << db) | (value - vmin), sorted ascending, so one
// sort does the grouping and the ordering.  Both files instantiate these bodies; the arithmetic of
// the pick exists once.
#pragma once
#include "mr_internal.h"

// [start, end) of each group in the sorted keys; off / endp zeroed by the caller (a group without
// keys keeps 0, 0), one slot per group value a key can carry
__device__ __forceinline__ void q_bounds_body(const uint64_t* key, int64_t S, int db, int64_t* off, int64_t* endp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const uint64_t k = key[i] >> db;
    if (i == 0 || (key[i - 1] >> db) != k) off[k] = i;
    if (i == S - 1 || (key[i + 1] >> db) != k) endp[k] = i + 1;
}

// numpy 2.x _quantile for integer data: vi = (n - 1) * q; lower / higher take a[floor / ceil];
// linear is _lerp(a[p], a[nx], g) with the int64 difference converted once and the result taken
// from the upper end when g >= 0.5.  (-ffp-contract=off: no multiply-add fuses here.)
// One thread per (group, quantile): out[t], and count[group] from the thread of quantile 0.
__device__ __forceinline__ void q_pick_body(const uint64_t* key, const int64_t* off, const int64_t* endp, int64_t n_groups,
                                            const double* q, int32_t n_q, int method, int64_t vmin, int db, double* out,
                                            int64_t* count) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_groups * n_q) return;
    const int64_t o = t / n_q;
    const int32_t j = (int32_t)(t % n_q);
    const int64_t beg = off[o], n = endp[o] - beg;
    if (j == 0) count[o] = n;
    if (n <= 0) {
        out[t] = 0.0;
        return;
    }
    const uint64_t mask = db ? (~0ull >> (64 - db)) : 0ull;
    const double vi = (double)(n - 1) * q[j];
    const double fl = floor(vi);
    int64_t p, nx;
    if (method == MR_Q_LOWER) {
        p = nx = (int64_t)fl;
    } else if (method == MR_Q_HIGHER) {
        p = nx = (int64_t)ceil(vi);
    } else {
        p = (int64_t)fl;
        nx = p + 1;
        if (vi >= (double)(n - 1)) p = nx = n - 1;
    }
    p = p < 0 ? 0 : (p > n - 1 ? n - 1 : p);   // (q in [0, 1] keeps both inside; never read past the group)
    nx = nx < 0 ? 0 : (nx > n - 1 ? n - 1 : nx);
    const int64_t ap = (int64_t)((key[beg + p] & mask) + (uint64_t)vmin);
    if (method != MR_Q_LINEAR) {
        out[t] = (double)ap;
        return;
    }
    const int64_t an = (int64_t)((key[beg + nx] & mask) + (uint64_t)vmin);
    const double g = vi - fl;
    const double diff = (double)(an - ap);
    double r = (double)ap + diff * g;
    if (g >= 0.5) r = (double)an - diff * (1.0 - g);
    out[t] = r;
}
