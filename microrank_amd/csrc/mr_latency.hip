// Latency evidence for a ranked window's top ops (no reference counterpart): per asked pod-op and
// side of the detector's partition (normal / abnormal traces) the row count and numpy.quantile of
// the rows' duration or SELF time, self = duration - csum[span], csum[c] the summed duration of the
// rows whose parent is span code c (T11's join: traceID ignored, int64 sums that wrap).
//
// mr_quantile.hip's design -- one sort of packed keys does the grouping and the ordering -- over the
// SELECTED rows only (a top list's ops hold ~1 % of a table's rows):
//   k_lat_csum    once per table (MR_LAT_SELF): runs of equal parents inside a wave are summed by a
//                 segmented wave scan, one 64-bit integer atomic add per run (order-free sums)
//   k_lat_select  <false>: count, min and max of the selected values of every window of the call
//                 (one launch; one read-back sizes the key buffer and the key width);
//                 <true>: key = class << DB | (value - vmin) for the selected rows, appended through
//                 one atomic per wave (the order is free: the sort carries keys only)
//                 class = (window * K + slot) * 2 + side; the asked codes of a window sit in LDS
//   mr_radix_sort, k_lat_bounds, k_lat_pick: ONE sort, one bounds pass and one pick launch for the
//                 whole call; the order-statistic arithmetic is mr_quantile_dev.h's
// DB = bits of (vmax - vmin); bits(n_windows * K * 2) + DB > 64 is MR_ERR_ARG.  mr_windows_latency's
// window list goes through mr_evidence.h's front end (each window's detector synchronises).
#include <climits>

#include "mr_evidence.h"
#include "mr_quantile_dev.h"
#include "mr_sort.h"

namespace {
constexpr int LT = 256;            // threads per block
constexpr int LAT_MAXB = 1024;     // k_lat_select blocks per window (grid-stride)
constexpr int LAT_MAX_OPS = 64;    // asked ops per window (mr_graph_exemplars' op limit)
constexpr int LAT_MAX_Y = 32768;   // windows per k_lat_select launch (gridDim.y)

struct LatWin {
    const int32_t *podop, *trace;
    const int64_t *dur, *span, *ts, *te;   // ts == nullptr: no test of the row's own times
    const unsigned long long* csum;        // nullptr: MR_LAT_DURATION
    const uint8_t* state;
    int64_t S, t0, t1, n_codes, cls0;      // cls0 = window * K * 2
    int32_t n_traces, n_ops;               // n_ops distinct asked codes (0: nothing is selected)
    int32_t ops[LAT_MAX_OPS];
};

// csum[parent[i]] += duration[i].  A span's children are mostly adjacent rows, so a per-row atomic
// would serialise lanes on one address: each run of equal parents among consecutive lanes is summed
// (wave_run_reduce) and its last lane alone issues the atomic.  uint64 adds: int64 sums that wrap,
// whatever the arrival order.
struct LatSum {
    unsigned long long v;
    __device__ __forceinline__ LatSum up(int off) const { return LatSum{__shfl_up(v, off, WAVE)}; }
    __device__ __forceinline__ void merge(const LatSum& lower) { v += lower.v; }
};
__global__ void __launch_bounds__(LT) k_lat_csum(const int64_t* parent, const int64_t* dur, int64_t S, int64_t n_codes,
                                                 unsigned long long* csum) {
    const int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    int64_t p = i < S ? parent[i] : -1;
    if (p < 0 || p >= n_codes) p = -1;   // no parent / an orphan's code: contributes nothing
    LatSum sum{p >= 0 ? (unsigned long long)dur[i] : 0ull};
    const bool tail = wave_run_reduce(lane, p, sum);
    if (p >= 0 && tail) atomicAdd(&csum[p], sum.v);
}

// words: [0] selected rows (COUNT) / append cursor (WRITE), [1] min, [2] max of the selected values
template <bool WRITE>
__global__ void __launch_bounds__(LT) k_lat_select(const LatWin* ws, long long vmin, int db, unsigned long long* words,
                                                   uint64_t* key, int64_t cap) {
    __shared__ int32_t ops[LAT_MAX_OPS];
    __shared__ long long rmin[LT / WAVE], rmax[LT / WAVE], rcnt[LT / WAVE];
    const LatWin* w = ws + blockIdx.y;
    const int32_t n = w->n_ops;
    if (threadIdx.x < LAT_MAX_OPS) ops[threadIdx.x] = (int)threadIdx.x < n ? w->ops[threadIdx.x] : -1;
    __syncthreads();
    if (n == 0) return;   // (block-uniform) an empty window, or none asked
    const int32_t *podop = w->podop, *trace = w->trace;
    const int64_t *dur = w->dur, *span = w->span, *ts = w->ts, *te = w->te;
    const unsigned long long* csum = w->csum;
    const uint8_t* state = w->state;
    const int64_t S = w->S, t0 = w->t0, t1 = w->t1, n_codes = w->n_codes, cls0 = w->cls0;
    const int32_t n_traces = w->n_traces;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t G = (S + 3) >> 2;   // four rows per thread: one 16-byte load of pod-op codes
    long long lo = LLONG_MAX, hi = LLONG_MIN, cnt = 0;
    for (int64_t g0 = (int64_t)blockIdx.x * LT; g0 < G; g0 += (int64_t)gridDim.x * LT) {   // (block-uniform trips)
        const int64_t base = (g0 + threadIdx.x) << 2;
        int32_t p[4] = {-1, -1, -1, -1};
        if (base + 3 < S) {
            const int4 v4 = *reinterpret_cast<const int4*>(podop + base);
            p[0] = v4.x, p[1] = v4.y, p[2] = v4.z, p[3] = v4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (base + k < S) p[k] = podop[base + k];
        }
        bool sel[4];
        long long val[4];
        int64_t cls[4];
        int c = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sel[k] = false;
            val[k] = 0;
            cls[k] = 0;
            int slot = -1;
            if (p[k] >= 0)
                for (int j = 0; j < n; ++j)
                    if (ops[j] == p[k]) slot = j;   // (the asked codes are distinct)
            if (slot < 0) continue;
            const int64_t i = base + k;
            const int32_t t = trace[i];
            if ((uint32_t)t >= (uint32_t)n_traces) continue;
            const int st = state[t];
            if (st != 1 && st != 2) continue;
            if (ts && !(ts[i] >= t0 && te[i] <= t1)) continue;
            unsigned long long v = (unsigned long long)dur[i];
            if (csum) {
                const int64_t sc = span[i];
                if (sc >= 0 && sc < n_codes) v -= csum[sc];
            }
            sel[k] = true;
            val[k] = (long long)v;
            cls[k] = cls0 + slot * 2 + (st - 1);
            ++c;
        }
        if (!WRITE) {
            cnt += c;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (sel[k]) {
                    lo = val[k] < lo ? val[k] : lo;
                    hi = val[k] > hi ? val[k] : hi;
                }
        } else {
            int inc = c;   // inclusive scan of the lanes' counts: one append per wave
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const int o = __shfl_up(inc, off, WAVE);
                if (lane >= off) inc += o;
            }
            const int total = __shfl(inc, WAVE - 1, WAVE);
            if (total) {   // (wave-uniform)
                unsigned long long b = 0;
                if (lane == 0) b = atomicAdd(&words[0], (unsigned long long)total);
                b = __shfl(b, 0, WAVE);
                int64_t pos = (int64_t)b + inc - c;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (sel[k]) {
                        if (pos < cap) key[pos] = ((uint64_t)cls[k] << db) | ((uint64_t)val[k] - (uint64_t)vmin);
                        ++pos;
                    }
            }
        }
    }
    if (WRITE) return;
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const long long a = __shfl_xor(lo, m, WAVE), b = __shfl_xor(hi, m, WAVE);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        cnt += __shfl_xor(cnt, m, WAVE);
    }
    const int wv = threadIdx.x / WAVE;
    if (lane == 0) {
        rmin[wv] = lo;
        rmax[wv] = hi;
        rcnt[wv] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < LT / WAVE; ++i) {
            lo = rmin[i] < lo ? rmin[i] : lo;
            hi = rmax[i] > hi ? rmax[i] : hi;
            cnt += rcnt[i];
        }
        if (cnt) {   // this block selected a row
            atomicAdd(&words[0], (unsigned long long)cnt);
            atomicMin((long long*)&words[1], lo);
            atomicMax((long long*)&words[2], hi);
        }
    }
}

// off / endp hold one slot per class, zeroed by the caller
__global__ void k_lat_bounds(const uint64_t* key, int64_t n, int db, int64_t* off, int64_t* endp) {
    q_bounds_body(key, n, db, off, endp);
}

__global__ void k_lat_pick(const uint64_t* key, const int64_t* off, const int64_t* endp, int64_t n_cls, const double* q,
                           int32_t n_q, int method, int64_t vmin, int db, double* out, int64_t* count) {
    q_pick_body(key, off, endp, n_cls, q, n_q, method, vmin, db, out, count);
}

// one window of a call: its table, its bounds, its partition on the device and its asked codes
struct LatReq {
    const mr_spans* s;
    int64_t t0, t1;
    const uint8_t* d_state;
    bool by_state;          // the state alone says which rows are inside [t0, t1]
    const int32_t* ops;     // (host) n_ops asked codes, checked by the caller
    int32_t n_ops;
};

}  // namespace

// (mr_internal.h: mr_timeline.hip's MR_LAT_SELF reads the same buffer)
int lat_csum_ensure(mr_ctx* ctx, const mr_spans* s) {
    if (s->csum_ok) return MR_OK;
    MR_TRY(s->csum.zero(ctx, (size_t)std::max<int64_t>(s->n_span_codes, 1)));
    if (s->S && s->n_span_codes)
        hipLaunchKernelGGL(k_lat_csum, dim3(cdiv(s->S, LT)), dim3(LT), 0, ctx->stream, s->parent.p, s->duration.p, s->S,
                           s->n_span_codes, s->csum.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    s->csum_ok = true;   // (stream-ordered: every reader is enqueued behind it on the context's stream)
    return MR_OK;
}

// the arguments both entries share (mr_internal.h: mr_windows_timeline_q checks its own the same way)
int lat_args(mr_ctx* ctx, const char* who, int what, const double* q, int32_t n_q, int method) {
    if (n_q < 1 || n_q > LAT_MAX_Q) return mr_fail(ctx, MR_ERR_ARG, "%s: n_q = %d is not in 1..%d", who, n_q, LAT_MAX_Q);
    if (what != MR_LAT_DURATION && what != MR_LAT_SELF) return mr_fail(ctx, MR_ERR_ARG, "%s: unknown what %d", who, what);
    if (method != MR_Q_LINEAR && method != MR_Q_LOWER && method != MR_Q_HIGHER)
        return mr_fail(ctx, MR_ERR_ARG, "%s: unknown method %d", who, method);
    for (int32_t j = 0; j < n_q; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0))   // (false for NaN)
            return mr_fail(ctx, MR_ERR_ARG, "%s: q[%d] = %g is not in [0, 1]", who, j, q[j]);
    return MR_OK;
}

namespace {

// out [nw * K * 2 * n_q] and count [nw * K * 2] (host), zeroed by the caller
int lat_run(mr_ctx* ctx, const char* who, int64_t nw, const LatReq* rq, int32_t K, int what, const double* q, int32_t n_q,
            int method, double* out, int64_t* count) {
    hipStream_t st = ctx->stream;
    std::vector<LatWin> hw((size_t)nw);   // (rep: the slot whose classes answer an asked entry)
    std::vector<int32_t> rep((size_t)nw * K, -1);
    int64_t maxS = 0;
    for (int64_t i = 0; i < nw; ++i) {
        const LatReq& r = rq[i];
        const mr_spans* s = r.s;
        LatWin& w = hw[(size_t)i];
        const bool whole = r.t0 == INT64_MIN && r.t1 == INT64_MAX;
        if (what == MR_LAT_SELF && r.n_ops) MR_TRY(lat_csum_ensure(ctx, s));
        w = LatWin{s->podop.p, s->trace.p, s->duration.p, s->span.p, (whole || r.by_state) ? nullptr : s->tstart.p,
                   (whole || r.by_state) ? nullptr : s->tend.p, what == MR_LAT_SELF ? s->csum.p : nullptr, r.d_state, s->S,
                   r.t0, r.t1, s->n_span_codes, i * K * 2, s->n_traces, 0, {}};
        ev_slots(r.ops, r.n_ops, w.ops, &w.n_ops, nullptr, &rep[(size_t)(i * K)]);
        if (s->S == 0) w.n_ops = 0;
        if (w.n_ops) maxS = std::max(maxS, s->S);
    }
    if (maxS == 0) return MR_OK;   // nothing can be selected: every count is 0
    const int64_t NC = nw * K * 2;
    const int cb = bits_for((uint64_t)NC);
    DBuf<LatWin> dw;
    DBuf<int64_t> words;
    MR_TRY(dw.upload(ctx, hw.data(), (size_t)nw));
    const int64_t init[3] = {0, INT64_MAX, INT64_MIN};
    MR_TRY(words.upload(ctx, init, 3));
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv(cdiv(maxS, 4), LT), LAT_MAXB);
    for (int64_t y0 = 0; y0 < nw; y0 += LAT_MAX_Y)
        hipLaunchKernelGGL(k_lat_select<false>, dim3(gx, (unsigned)std::min<int64_t>(nw - y0, LAT_MAX_Y)), dim3(LT), 0, st,
                           dw.p + y0, 0ll, 0, (unsigned long long*)words.p, (uint64_t*)nullptr, (int64_t)0);
    MR_TRY_HIP(ctx, hipGetLastError());
    int64_t h[3];
    MR_TRY(mr_read_words(ctx, words.p, 3, h));   // (syncs: hw and init are no longer read)
    const int64_t total = h[0];
    if (total == 0) return MR_OK;
    const int64_t vmin = h[1];
    const int db = bits_for((uint64_t)h[2] - (uint64_t)h[1]);
    if (cb + db > 64)
        return mr_fail(ctx, MR_ERR_ARG,
                       "%s: value range too wide to sort (%lld .. %lld needs %d bits beside %d class bits; 64 in all)", who,
                       (long long)h[1], (long long)h[2], db, cb);
    DBuf<uint64_t> key;
    DBuf<int64_t> off, endp, dc;
    DBuf<double> dq, dout;
    SortScratch ws;
    const int64_t NQ = NC * n_q;
    MR_TRY(key.alloc(ctx, (size_t)total));
    MR_TRY(off.zero(ctx, (size_t)NC + 1));
    MR_TRY(endp.zero(ctx, (size_t)NC + 1));
    MR_TRY(dq.upload(ctx, q, (size_t)n_q));
    MR_TRY(dout.alloc(ctx, (size_t)NQ));
    MR_TRY(dc.alloc(ctx, (size_t)NC));
    MR_TRY_HIP(ctx, hipMemsetAsync(words.p, 0, sizeof(int64_t), st));   // the append cursor
    for (int64_t y0 = 0; y0 < nw; y0 += LAT_MAX_Y)
        hipLaunchKernelGGL(k_lat_select<true>, dim3(gx, (unsigned)std::min<int64_t>(nw - y0, LAT_MAX_Y)), dim3(LT), 0, st,
                           dw.p + y0, (long long)vmin, db, (unsigned long long*)words.p, key.p, total);
    MR_TRY(mr_radix_sort(ctx, key.p, nullptr, total, cb + db, ws));
    hipLaunchKernelGGL(k_lat_bounds, dim3(cdiv(total, LT)), dim3(LT), 0, st, key.p, total, db, off.p, endp.p);
    hipLaunchKernelGGL(k_lat_pick, dim3(cdiv(NQ, LT)), dim3(LT), 0, st, key.p, off.p, endp.p, NC, dq.p, n_q, method, vmin,
                       db, dout.p, dc.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    std::vector<double> ho((size_t)NQ);
    std::vector<int64_t> hc((size_t)NC);
    MR_TRY(dout.download(ctx, ho.data(), (size_t)NQ));
    MR_TRY(dc.download(ctx, hc.data(), (size_t)NC));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));   // (q, the sort's scratch and the keys leave scope)
    for (int64_t i = 0; i < nw; ++i)
        for (int32_t j = 0; j < rq[i].n_ops; ++j) {
            if (hw[(size_t)i].n_ops == 0) continue;
            const int64_t dst = (i * K + j) * 2, src = (i * K + rep[(size_t)(i * K + j)]) * 2;
            for (int side = 0; side < 2; ++side) {
                count[dst + side] = hc[(size_t)(src + side)];
                for (int32_t k = 0; k < n_q; ++k) out[(dst + side) * n_q + k] = ho[(size_t)((src + side) * n_q + k)];
            }
        }
    return MR_OK;
}
}  // namespace

extern "C" int mr_op_latency(mr_ctx* ctx, const mr_spans* s, int64_t t0, int64_t t1, const uint8_t* state,
                             const int32_t* podops, int32_t n_ops, int what, const double* q, int32_t n_q, int method,
                             double* out, int64_t* count) {
    if (!ctx || !s || s->ctx != ctx || !state || !podops || !q || !out || !count)
        return mr_fail(ctx, MR_ERR_ARG, "mr_op_latency: bad arguments");
    if (n_ops < 1 || n_ops > LAT_MAX_OPS)
        return mr_fail(ctx, MR_ERR_ARG, "mr_op_latency: n_ops = %d is not in 1..%d", n_ops, LAT_MAX_OPS);
    MR_TRY(lat_args(ctx, "mr_op_latency", what, q, n_q, method));
    for (int32_t j = 0; j < n_ops; ++j)
        if (podops[j] < 0 || podops[j] >= s->n_podops)
            return mr_fail(ctx, MR_ERR_ARG, "mr_op_latency: podops[%d] = %d is no pod-op code of the table (%d)", j,
                           podops[j], s->n_podops);
    const bool whole = t0 == INT64_MIN && t1 == INT64_MAX;
    if (!whole && !s->has_times)
        return mr_fail(ctx, MR_ERR_STATE, "mr_op_latency: a window needs startTime/endTime columns");
    if (what == MR_LAT_SELF && s->grow.p)
        return mr_fail(ctx, MR_ERR_STATE, "mr_op_latency: self time on a shard of a larger table (children may lie on another rank)");
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    std::fill(out, out + (size_t)n_ops * 2 * n_q, 0.0);
    std::fill(count, count + (size_t)n_ops * 2, (int64_t)0);
    DBuf<uint8_t> dst;
    MR_TRY(dst.upload(ctx, state, (size_t)s->n_traces));
    // (a caller's state says nothing about the window: the rows' own times are tested)
    const LatReq r{s, t0, t1, dst.p, false, podops, n_ops};
    MR_TRY(lat_run(ctx, "mr_op_latency", 1, &r, n_ops, what, q, n_q, method, out, count));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (state was read)
    return MR_OK;
}

extern "C" int mr_windows_latency(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                  const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                  const int32_t* podops, const int32_t* n_ops, int32_t K, int what, const double* q,
                                  int32_t n_q, int method, double* out, int64_t* count, int32_t* status) {
    const char* who = "mr_windows_latency";
    const EvList L{n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K};
    MR_TRY(ev_check_args(ctx, who, L, q && (!n_windows || (out && count && status)), LAT_MAX_OPS));
    MR_TRY(lat_args(ctx, who, what, q, n_q, method));
    MR_TRY(ev_check_windows(ctx, who, L, false));
    for (int32_t i = 0; i < n_windows; ++i) {
        if (!spans[i]->has_times) return mr_fail(ctx, MR_ERR_STATE, "%s: window %d needs startTime/endTime columns", who, i);
        if (what == MR_LAT_SELF && spans[i]->grow.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: self time on a shard of a larger table", who, i);
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (n_windows == 0) return MR_OK;
    std::fill(out, out + (size_t)n_windows * K * 2 * n_q, 0.0);
    std::fill(count, count + (size_t)n_windows * K * 2, (int64_t)0);
    std::fill(status, status + n_windows, (int32_t)MR_OK);
    // the windows' detectors, one after another (mr_evidence.h); each partition stays on the device
    EvSlos slos;
    std::vector<DBuf<uint8_t>> dst((size_t)n_windows);
    std::vector<LatReq> rq((size_t)n_windows);
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        bool launched = false, empty = false;
        MR_TRY(ev_partition(ctx, L, i, slos, dst[(size_t)i], nullptr, &launched, &empty, status));
        rq[(size_t)i] = LatReq{s, t0[i], t1[i], dst[(size_t)i].p, s->indexed && s->uniform_times,
                               podops + (size_t)i * K, empty ? 0 : n_ops[i]};
    }
    MR_TRY(lat_run(ctx, who, n_windows, rq.data(), K, what, q, n_q, method, out, count));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the states and the SLO arrays leave scope)
    return MR_OK;
}
