// K4 extension: per-service-op duration quantiles (numpy.quantile semantics) on gfx950.
// No reference counterpart: extends preprocess_data.get_operation_slo (preprocess_data.py:50-78)
// with a percentile baseline, returned to the detector as [Q, 0.0] so mean + 3 * std is Q.
//
// One sort of packed keys does the grouping and the ordering:
//   k_q_range   min / max duration of the rows that take part (wave shuffles, LDS per block, one
//               64-bit atomic min and max per block); read back once for the key width
//   k_q_keys    key = (op << DB) | (duration - dmin); rows outside the window carry the op code
//               n_svcops, so they sort behind every op
//   mr_radix_sort on the low OB + DB bits (no value payload)
//   k_q_bounds  [start, end) of each op in the sorted keys (as k_slo_count does)
//   k_q_pick    one thread per (op, quantile): numpy 2.x's _quantile arithmetic on the one or two
//               order statistics it needs, restored from the keys (mr_quantile_dev.h, shared with
//               mr_latency.hip)
// DB = bits of (dmax - dmin), OB = bits of n_svcops; OB + DB > 64 is MR_ERR_ARG.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "mr_prim.h"
#include "mr_quantile_dev.h"
#include "mr_sort.h"

namespace {
constexpr int QT = 256;          // threads per block
constexpr int Q_RANGE_MAXB = 1024;   // k_q_range blocks (grid-stride)

__device__ __forceinline__ bool q_in_window(const int64_t* ts, const int64_t* te, int64_t i, int64_t t0, int64_t t1) {
    return !ts || (ts[i] >= t0 && te[i] <= t1);   // ts == nullptr: the whole table
}

// mm[0] = min, mm[1] = max (preset to INT64_MAX / INT64_MIN: no row leaves min > max)
__global__ void __launch_bounds__(QT) k_q_range(const int64_t* dur, const int64_t* ts, const int64_t* te, int64_t S,
                                                int64_t t0, int64_t t1, long long* mm) {
    __shared__ long long rmin[QT / WAVE], rmax[QT / WAVE];
    long long lo = LLONG_MAX, hi = LLONG_MIN;
    for (int64_t i = (int64_t)blockIdx.x * QT + threadIdx.x; i < S; i += (int64_t)gridDim.x * QT) {
        if (!q_in_window(ts, te, i, t0, t1)) continue;
        const long long d = dur[i];
        lo = d < lo ? d : lo;
        hi = d > hi ? d : hi;
    }
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const long long a = __shfl_xor(lo, m, WAVE), b = __shfl_xor(hi, m, WAVE);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (lane == 0) {
        rmin[w] = lo;
        rmax[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < QT / WAVE; ++i) {
            lo = rmin[i] < lo ? rmin[i] : lo;
            hi = rmax[i] > hi ? rmax[i] : hi;
        }
        if (lo <= hi) {   // this block saw a row
            atomicMin(&mm[0], lo);
            atomicMax(&mm[1], hi);
        }
    }
}

__global__ void k_q_keys(const int32_t* svcop, const int64_t* dur, const int64_t* ts, const int64_t* te, int64_t S,
                         int64_t t0, int64_t t1, int32_t n_ops, int64_t dmin, int db, uint64_t* key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const uint32_t op = (uint32_t)svcop[i];
    if (op < (uint32_t)n_ops && q_in_window(ts, te, i, t0, t1))
        key[i] = ((uint64_t)op << db) | ((uint64_t)dur[i] - (uint64_t)dmin);
    else
        key[i] = (uint64_t)(uint32_t)n_ops << db;
}

// off / endp hold n_ops + 1 slots (the last one is the sentinel's), zeroed by the caller
__global__ void k_q_bounds(const uint64_t* key, int64_t S, int db, int64_t* off, int64_t* endp) {
    q_bounds_body(key, S, db, off, endp);
}

// one thread per (op, quantile): numpy 2.x's _quantile arithmetic (mr_quantile_dev.h)
__global__ void k_q_pick(const uint64_t* key, const int64_t* off, const int64_t* endp, int32_t n_ops, const double* q,
                         int32_t n_q, int method, int64_t dmin, int db, double* out, int64_t* count) {
    q_pick_body(key, off, endp, n_ops, q, n_q, method, dmin, db, out, count);
}
}  // namespace

extern "C" int mr_slo_quantiles(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1, const double* q, int32_t n_q,
                                int method, double* out, int64_t* count) {
    if (!ctx || !s || s->ctx != ctx || !q || !out || !count || n_q < 1)
        return mr_fail(ctx, MR_ERR_ARG, "mr_slo_quantiles: bad arguments");
    if (method != MR_Q_LINEAR && method != MR_Q_LOWER && method != MR_Q_HIGHER)
        return mr_fail(ctx, MR_ERR_ARG, "mr_slo_quantiles: unknown method %d", method);
    for (int32_t j = 0; j < n_q; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0))   // (false for NaN)
            return mr_fail(ctx, MR_ERR_ARG, "mr_slo_quantiles: q[%d] = %g is not in [0, 1]", j, q[j]);
    const bool whole = t0 == INT64_MIN && t1 == INT64_MAX;
    if (!whole && !s->has_times)
        return mr_fail(ctx, MR_ERR_STATE, "mr_slo_quantiles: a window needs startTime/endTime columns");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t S = s->S;
    const int32_t NO = s->n_svcops;
    if (NO == 0) return MR_OK;
    const int64_t* ts = whole ? nullptr : s->tstart.p;
    const int64_t* te = whole ? nullptr : s->tend.p;
    const int64_t NQ = (int64_t)NO * n_q;

    int64_t dmin = 0;
    int db = 0;
    bool any = false;
    if (S) {
        const int64_t init[2] = {INT64_MAX, INT64_MIN};
        int64_t h[2];
        DBuf<int64_t> mm;
        MR_TRY(mm.upload(ctx, init, 2));
        hipLaunchKernelGGL(k_q_range, dim3((unsigned)std::min<int64_t>(cdiv(S, QT), Q_RANGE_MAXB)), dim3(QT), 0, st,
                           s->duration.p, ts, te, S, t0, t1, (long long*)mm.p);
        MR_TRY_HIP(ctx, hipGetLastError());
        MR_TRY(mr_read_words(ctx, mm.p, 2, h));   // (syncs: init is no longer read)
        any = h[0] <= h[1];
        if (any) {
            dmin = h[0];
            db = bits_for((uint64_t)h[1] - (uint64_t)h[0]);
            if (bits_for((uint64_t)NO) + db > 64)
                return mr_fail(ctx, MR_ERR_ARG,
                               "mr_slo_quantiles: duration range too wide to sort (%lld .. %lld needs %d bits beside %d "
                               "op bits; 64 in all)",
                               (long long)h[0], (long long)h[1], db, bits_for((uint64_t)NO));
        }
    }
    const int ob = bits_for((uint64_t)NO);
    DBuf<uint64_t> key;
    DBuf<int64_t> off, endp, dc;
    DBuf<double> dq, dout;
    SortScratch ws;
    MR_TRY(off.zero(ctx, (size_t)NO + 1));
    MR_TRY(endp.zero(ctx, (size_t)NO + 1));
    MR_TRY(dq.upload(ctx, q, (size_t)n_q));
    MR_TRY(dout.alloc(ctx, (size_t)NQ));
    MR_TRY(dc.alloc(ctx, (size_t)NO));
    if (any) {
        MR_TRY(key.alloc(ctx, (size_t)S));
        hipLaunchKernelGGL(k_q_keys, dim3(cdiv(S, QT)), dim3(QT), 0, st, s->svcop.p, s->duration.p, ts, te, S, t0, t1, NO,
                           dmin, db, key.p);
        MR_TRY(mr_radix_sort(ctx, key.p, nullptr, S, ob + db, ws));
        hipLaunchKernelGGL(k_q_bounds, dim3(cdiv(S, QT)), dim3(QT), 0, st, key.p, S, db, off.p, endp.p);
    }
    hipLaunchKernelGGL(k_q_pick, dim3(cdiv(NQ, QT)), dim3(QT), 0, st, key.p, off.p, endp.p, NO, dq.p, n_q, method, dmin,
                       db, dout.p, dc.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY(dout.download(ctx, out, (size_t)NQ));
    MR_TRY(dc.download(ctx, count, (size_t)NO));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (q, the sort's scratch and the keys leave scope)
    return MR_OK;
}
