// Timeline evidence of a window (no reference counterpart): per asked pod-op -- and for the window as a
// whole -- a dense histogram over time buckets of the rows' (or traces') count, summed value and largest
// value, on the normal and on the abnormal side of the window's own detector partition.  The other
// evidence entries collapse the window's time axis; this one says WHEN: whether the anomaly is a burst
// that is over or still going on, and whether the suspect op got slow when the abnormal traces began.
//
// Everything it needs is on the device already: the detector's state byte per trace, the per-trace index's
// trace-level start and end (tts / tte), and the self-time evidence's csum (mr_latency.hip).  The answer is
// dense, so there is no join, no selection and no merge:
//   k_tl_count   one launch for a chunk's windows (gridDim.y).  Blocks [0, rb) of a window make the ROW
//                pass: a lane per row, TL_U rows in flight per lane: the row's trace state first (a row
//                outside the partition reads nothing more), then its pod-op and that code's slot among
//                the distinct asked codes (at most 64, in LDS, behind a 64-bit filter of code & 63 in
//                registers), then the trace's start, its bucket and the value -- for MR_LAT_SELF span and
//                csum, read only by rows that have a slot.  Blocks [rb, rb + tb) make the TRACE pass of
//                slot -1: a lane per trace code, its state, start and end.  Both feed one reduction:
//                key = (slot * (B + 2) + bucket) * 2 + side, buckets B and B + 1 standing for "before" and
//                "after" the bucket range.  Runs of equal keys inside a wave are reduced (mr_prim.h
//                wave_run_reduce; a wave without a key skips it) and the run's last lane adds n, the sum
//                and the maximum to the block's counter table in LDS (mr_evidence.h EvTable), direct-mapped
//                where the window's distinct asked * (B + 2) * 2 keys fit, else hashed.  The block adds its
//                table to the window's dense counters once, at its end.  The counters are bitwise
//                reproducible, whatever the cut and whichever path a run took
//   k_tl_finish  a thread per output word: the counters of the slot that answers an asked entry (a
//                duplicate: its first appearance's), the maximum un-biased and 0 where the count is 0, the
//                two outside buckets into tl_out
// One row pass and one trace pass per chunk of windows -- never a launch per asked op or per bucket -- and
// one pinned read-back per chunk, which carries the detectors' counts too: no host synchronisation per
// window.  The window list's front end is mr_evidence.h's; a chunk's dense counters take K * (B + 2) * 2 * 3
// words per window (MR_TL_CHUNK, read per call, forces the windows per chunk; MR_TL_BLOCKS the blocks
// per window of each pass: tests reach every cut at small sizes).
//
// mr_windows_timeline_q adds np.quantile per (asked entry, bucket, side) to the same chunk, from the same
// partitions -- mr_latency.hip's design with the bucket in the class:
//   k_tlq_select  k_tl_count's two passes with its order of reads, emitting instead of counting: <false> the
//                 chunk's selected total, minimum and maximum (buckets inside the range only; ONE read-back
//                 sizes the key buffer and the key width), <true> key = class << db | (value - vmin), class =
//                 ((window in chunk * n_slots_max + slot) * B + bucket) * 2 + side, appended through one
//                 atomic per wave and tile (the order is free: the sort carries keys only)
//   mr_radix_sort, k_tlq_bounds, k_tlq_pick (mr_quantile_dev.h's bodies): ONE sort over class bits + db bits,
//                 one bounds and one pick launch for the chunk; bits(classes - 1) + db > 64 is MR_ERR_ARG
//   k_tlq_gather  a thread per tl_q word: the class of the slot that answers the entry, 0.0 for no slot
// Integer until the pick, so tl_q is the same bits under every cut; it rides in the chunk's one read-back.
#include <climits>

#include "mr_evidence.h"
#include "mr_quantile_dev.h"
#include "mr_sort.h"

namespace {
constexpr int TL_T = 256;                     // threads per block
constexpr int TL_U = 4;                       // k_tl_count: rows (traces) in flight per lane
constexpr int TL_TILE = TL_T * TL_U;          // rows of a block's tile
constexpr int TL_MAXOPS = 64;                 // asked slots per window (the evidence entries' limit)
constexpr int TL_MAXB = 512;                  // buckets
constexpr int TL_MAX_CB = 4096;               // row blocks per window (grid-stride over the tiles)

struct TlWin {
    const int32_t *podop, *trace;
    const int64_t *dur, *span;
    const long long *tts, *tte;           // [NT] trace-level start / end (the per-trace index's)
    const unsigned long long* csum;       // nullptr: MR_LAT_DURATION
    const uint8_t* state;
    unsigned long long* cnt;              // [K * (B + 2) * 2 * 3]: slot, bucket, side, {n, sum, biased max}
    int64_t S, n_codes;                   // S: the rows of the row pass (0: no op slot asked)
    long long b0;
    unsigned long long bw;
    int32_t NT, NTp;                      // traces of the table; of the trace pass (0: -1 not asked)
    int32_t n_ops, all_slot;              // distinct asked slots; the slot of -1 (or -1: not asked)
    int32_t direct;                       // the keys fit the block's table: direct-mapped
    int32_t op[TL_MAXOPS];                // asked codes by slot (-1 at all_slot)
};

// the bucket of a start: B "before", B + 1 "after" (delta is exact as uint64 since ts >= b0, for b0 = INT64_MIN too)
__device__ __forceinline__ int tl_bucket(long long ts, long long b0, unsigned long long bw, int B) {
    if (ts < b0) return B;
    const unsigned long long b = ((unsigned long long)ts - (unsigned long long)b0) / bw;
    return b >= (unsigned long long)B ? B + 1 : (int)b;
}

// every lane of the wave brings (kd, d), kd < 0: nothing; runs of equal keys are reduced and added once
__device__ __forceinline__ void tl_reduce(int lane, bool direct, EvTable& tab, unsigned long long* cnt, int32_t kd,
                                          unsigned long long d) {
    if (__ballot(kd >= 0) == 0ull) return;   // (wave-uniform)
    EvRun run = ev_run_of(kd >= 0, d);
    const bool tail = wave_run_reduce(lane, kd, run);
    if (kd >= 0 && tail) tab.add(direct, cnt, kd, run);
}

// blocks [0, rb) of a window: the row pass; [rb, gridDim.x): the trace pass of slot -1
__global__ void __launch_bounds__(TL_T) k_tl_count(const TlWin* __restrict__ ws, int32_t rb, int32_t B) {
    __shared__ EvTable tab;   // n, sum, biased max
    __shared__ int32_t ops[TL_MAXOPS];
    const TlWin& w = ws[blockIdx.y];
    const bool rows = (int32_t)blockIdx.x < rb;
    const int32_t bx = rows ? (int32_t)blockIdx.x : (int32_t)blockIdx.x - rb, nbx = rows ? rb : (int32_t)gridDim.x - rb;
    const int64_t N = rows ? w.S : (int64_t)w.NTp;
    if ((int64_t)bx * TL_TILE >= N) return;   // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const bool direct = w.direct != 0;
    const int32_t n_ops = w.n_ops, BB = B + 2;
    tab.clear(threadIdx.x, TL_T);
    if (threadIdx.x < TL_MAXOPS) ops[threadIdx.x] = (int)threadIdx.x < n_ops ? w.op[threadIdx.x] : -1;
    __syncthreads();
    const uint32_t NT = (uint32_t)w.NT;
    const long long b0 = w.b0;
    const unsigned long long bw = w.bw;
    if (rows) {
        uint64_t filter = 0;   // bit (code & 63) of every asked code
        for (int j = 0; j < n_ops; ++j)
            if (ops[j] >= 0) filter |= 1ull << (ops[j] & 63);
        const int64_t n_codes = w.n_codes;
        const unsigned long long* __restrict__ csum = w.csum;
        for (int64_t base = (int64_t)bx * TL_TILE; base < N; base += (int64_t)nbx * TL_TILE) {   // (block-uniform)
            int32_t tr[TL_U], po[TL_U];
            int st[TL_U];
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t c = base + k * TL_T + threadIdx.x;
                tr[k] = c < N ? w.trace[c] : -1;
            }
#pragma unroll
            for (int k = 0; k < TL_U; ++k) st[k] = (uint32_t)tr[k] < NT ? (int)w.state[tr[k]] : 0;
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t c = base + k * TL_T + threadIdx.x;
                po[k] = st[k] == 1 || st[k] == 2 ? w.podop[c] : -1;
            }
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t c = base + k * TL_T + threadIdx.x;
                int slot = -1;
                if (po[k] >= 0 && (filter >> (po[k] & 63) & 1ull))
                    for (int j = 0; j < n_ops; ++j)
                        if (ops[j] == po[k]) slot = j;   // (the asked codes are distinct)
                int32_t kd = -1;
                unsigned long long d = 0ull;
                if (slot >= 0) {
                    kd = (slot * BB + tl_bucket(w.tts[tr[k]], b0, bw, B)) * 2 + (st[k] - 1);
                    d = (unsigned long long)w.dur[c];
                    if (csum) {
                        const int64_t sc = w.span[c];
                        if (sc >= 0 && sc < n_codes) d -= csum[sc];
                    }
                }
                tl_reduce(lane, direct, tab, w.cnt, kd, d);
            }
        }
    } else {
        const int32_t all = w.all_slot;
        for (int64_t base = (int64_t)bx * TL_TILE; base < N; base += (int64_t)nbx * TL_TILE) {   // (block-uniform)
            int st[TL_U];
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t t = base + k * TL_T + threadIdx.x;
                st[k] = t < N ? (int)w.state[t] : 0;
            }
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t t = base + k * TL_T + threadIdx.x;
                int32_t kd = -1;
                unsigned long long d = 0ull;
                if (st[k] == 1 || st[k] == 2) {
                    const long long ts = w.tts[t];
                    kd = (all * BB + tl_bucket(ts, b0, bw, B)) * 2 + (st[k] - 1);
                    d = (unsigned long long)w.tte[t] - (unsigned long long)ts;
                }
                tl_reduce(lane, direct, tab, w.cnt, kd, d);
            }
        }
    }
    __syncthreads();
    tab.flush<int32_t>(direct, w.cnt, threadIdx.x, TL_T);
}

// word e < n1 = cw * K * B * 2 (window, asked entry, bucket, side): its count, sum and maximum; word n1 + e2,
// e2 < cw * K * 4 (window, asked entry, side, {before, after}): the count of that outside bucket.  rep[window *
// K + entry]: the slot that answers the entry, or -1 (not asked, or an empty window: zeros)
__global__ void __launch_bounds__(TL_T) k_tl_finish(const TlWin* __restrict__ ws, const int32_t* __restrict__ rep,
                                                    int32_t K, int32_t B, int64_t n1, int64_t n2,
                                                    long long* __restrict__ ocnt, long long* __restrict__ osum,
                                                    long long* __restrict__ omax, long long* __restrict__ oout) {
    const int64_t e = (int64_t)blockIdx.x * TL_T + threadIdx.x;
    const int32_t BB = B + 2;
    if (e < n1) {
        const int64_t per = (int64_t)K * B * 2;
        const int32_t wi = (int32_t)(e / per);
        const int32_t r = (int32_t)(e % per);
        const int32_t j = r / (B * 2), b = (r >> 1) % B, side = r & 1;
        const int32_t u = rep[(size_t)wi * K + j];
        long long c = 0, s = 0, x = 0;
        if (u >= 0) {
            const unsigned long long* p = ws[wi].cnt + (size_t)((u * BB + b) * 2 + side) * 3;
            c = (long long)p[0];
            s = (long long)p[1];
            x = c ? (long long)(p[2] ^ EV_BIAS) : 0ll;
        }
        ocnt[e] = c;
        osum[e] = s;
        omax[e] = x;
    } else if (e < n1 + n2) {
        const int64_t e2 = e - n1;
        const int32_t wi = (int32_t)(e2 / ((int64_t)K * 4));
        const int32_t r = (int32_t)(e2 % ((int64_t)K * 4));
        const int32_t j = r >> 2, side = (r >> 1) & 1, which = r & 1;
        const int32_t u = rep[(size_t)wi * K + j];
        oout[e2] = u >= 0 ? (long long)ws[wi].cnt[(size_t)((u * BB + B + which) * 2 + side) * 3] : 0ll;
    }
}
// ---------------------------------------------------------------- quantiles per bucket (mr_windows_timeline_q)
// A lane's TL_U candidates of a tile (c of them selected).  COUNT: into the lane's total, minimum and maximum.
// WRITE: key = class << db | (value - vmin) behind the cursor words[0], one atomic per wave and tile.
template <bool WRITE>
__device__ __forceinline__ void tlq_emit(int lane, const bool (&sel)[TL_U], const long long (&val)[TL_U],
                                         const uint64_t (&cls)[TL_U], int c, long long vmin, int db,
                                         unsigned long long* words, uint64_t* __restrict__ key, int64_t cap, long long& lo,
                                         long long& hi, long long& cnt) {
    if (!WRITE) {
        cnt += c;
#pragma unroll
        for (int k = 0; k < TL_U; ++k)
            if (sel[k]) {
                lo = val[k] < lo ? val[k] : lo;
                hi = val[k] > hi ? val[k] : hi;
            }
        return;
    }
    int inc = c;   // inclusive scan of the lanes' counts
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int o = __shfl_up(inc, off, WAVE);
        if (lane >= off) inc += o;
    }
    const int total = __shfl(inc, WAVE - 1, WAVE);
    if (total == 0) return;   // (wave-uniform)
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(&words[0], (unsigned long long)total);
    b = __shfl(b, 0, WAVE);
    int64_t pos = (int64_t)b + inc - c;
#pragma unroll
    for (int k = 0; k < TL_U; ++k)
        if (sel[k]) {
            if (pos < cap) key[pos] = (cls[k] << db) | ((uint64_t)val[k] - (uint64_t)vmin);
            ++pos;
        }
}

// k_tl_count's grid, passes and order of reads; words: [0] selected rows (COUNT) / append cursor (WRITE), [1] min,
// [2] max of the selected values.  Only buckets inside the range are selected.  nsm: the most distinct slots of
// a window of the chunk (the class stride)
template <bool WRITE>
__global__ void __launch_bounds__(TL_T) k_tlq_select(const TlWin* __restrict__ ws, int32_t rb, int32_t B, int32_t nsm,
                                                     long long vmin, int db, unsigned long long* words,
                                                     uint64_t* __restrict__ key, int64_t cap) {
    __shared__ int32_t ops[TL_MAXOPS];
    __shared__ long long rmin[TL_T / WAVE], rmax[TL_T / WAVE], rcnt[TL_T / WAVE];
    const TlWin& w = ws[blockIdx.y];
    const bool rows = (int32_t)blockIdx.x < rb;
    const int32_t bx = rows ? (int32_t)blockIdx.x : (int32_t)blockIdx.x - rb, nbx = rows ? rb : (int32_t)gridDim.x - rb;
    const int64_t N = rows ? w.S : (int64_t)w.NTp;
    if ((int64_t)bx * TL_TILE >= N) return;   // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const int32_t n_ops = w.n_ops;
    if (threadIdx.x < TL_MAXOPS) ops[threadIdx.x] = (int)threadIdx.x < n_ops ? w.op[threadIdx.x] : -1;
    __syncthreads();
    const uint32_t NT = (uint32_t)w.NT;
    const long long b0 = w.b0;
    const unsigned long long bw = w.bw;
    const uint64_t cls0 = (uint64_t)blockIdx.y * (uint64_t)nsm * (uint64_t)B * 2ull;
    long long lo = LLONG_MAX, hi = LLONG_MIN, cnt = 0;
    if (rows) {
        uint64_t filter = 0;   // bit (code & 63) of every asked code
        for (int j = 0; j < n_ops; ++j)
            if (ops[j] >= 0) filter |= 1ull << (ops[j] & 63);
        const int64_t n_codes = w.n_codes;
        const unsigned long long* __restrict__ csum = w.csum;
        for (int64_t base = (int64_t)bx * TL_TILE; base < N; base += (int64_t)nbx * TL_TILE) {   // (block-uniform)
            int32_t tr[TL_U], po[TL_U];
            int st[TL_U];
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t c = base + k * TL_T + threadIdx.x;
                tr[k] = c < N ? w.trace[c] : -1;
            }
#pragma unroll
            for (int k = 0; k < TL_U; ++k) st[k] = (uint32_t)tr[k] < NT ? (int)w.state[tr[k]] : 0;
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t c = base + k * TL_T + threadIdx.x;
                po[k] = st[k] == 1 || st[k] == 2 ? w.podop[c] : -1;
            }
            bool sel[TL_U];
            long long val[TL_U];
            uint64_t cls[TL_U];
            int n_sel = 0;
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t c = base + k * TL_T + threadIdx.x;
                sel[k] = false;
                val[k] = 0;
                cls[k] = 0;
                int slot = -1;
                if (po[k] >= 0 && (filter >> (po[k] & 63) & 1ull))
                    for (int j = 0; j < n_ops; ++j)
                        if (ops[j] == po[k]) slot = j;   // (the asked codes are distinct)
                if (slot < 0) continue;
                const int bk = tl_bucket(w.tts[tr[k]], b0, bw, B);
                if (bk >= B) continue;   // before / after: counted in tl_out, no quantiles
                unsigned long long d = (unsigned long long)w.dur[c];
                if (csum) {
                    const int64_t sc = w.span[c];
                    if (sc >= 0 && sc < n_codes) d -= csum[sc];
                }
                sel[k] = true;
                val[k] = (long long)d;
                cls[k] = cls0 + (uint64_t)((slot * B + bk) * 2 + (st[k] - 1));
                ++n_sel;
            }
            tlq_emit<WRITE>(lane, sel, val, cls, n_sel, vmin, db, words, key, cap, lo, hi, cnt);
        }
    } else {
        const int32_t all = w.all_slot;
        for (int64_t base = (int64_t)bx * TL_TILE; base < N; base += (int64_t)nbx * TL_TILE) {   // (block-uniform)
            int st[TL_U];
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t t = base + k * TL_T + threadIdx.x;
                st[k] = t < N ? (int)w.state[t] : 0;
            }
            bool sel[TL_U];
            long long val[TL_U];
            uint64_t cls[TL_U];
            int n_sel = 0;
#pragma unroll
            for (int k = 0; k < TL_U; ++k) {
                const int64_t t = base + k * TL_T + threadIdx.x;
                sel[k] = false;
                val[k] = 0;
                cls[k] = 0;
                if (st[k] != 1 && st[k] != 2) continue;
                const long long ts = w.tts[t];
                const int bk = tl_bucket(ts, b0, bw, B);
                if (bk >= B) continue;
                sel[k] = true;
                val[k] = (long long)((unsigned long long)w.tte[t] - (unsigned long long)ts);
                cls[k] = cls0 + (uint64_t)((all * B + bk) * 2 + (st[k] - 1));
                ++n_sel;
            }
            tlq_emit<WRITE>(lane, sel, val, cls, n_sel, vmin, db, words, key, cap, lo, hi, cnt);
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
        for (int i = 1; i < TL_T / WAVE; ++i) {
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
__global__ void k_tlq_bounds(const uint64_t* key, int64_t n, int db, int64_t* off, int64_t* endp) {
    q_bounds_body(key, n, db, off, endp);
}

__global__ void k_tlq_pick(const uint64_t* key, const int64_t* off, const int64_t* endp, int64_t n_cls, const double* q,
                           int32_t n_q, int method, int64_t vmin, int db, double* out, int64_t* count) {
    q_pick_body(key, off, endp, n_cls, q, n_q, method, vmin, db, out, count);
}

// word e < n = cw * K * B * 2 * n_q (window, asked entry, bucket, side, q): the pick of the class of the slot
// that answers the entry (rep, as k_tl_finish's), 0.0 for none.  pick: [class][n_q]
__global__ void __launch_bounds__(TL_T) k_tlq_gather(const int32_t* __restrict__ rep, const double* __restrict__ pick,
                                                     int32_t K, int32_t B, int32_t nsm, int32_t n_q, int64_t n,
                                                     double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * TL_T + threadIdx.x;
    if (e >= n) return;
    const int64_t slot_words = (int64_t)B * 2 * n_q, per = (int64_t)K * slot_words;
    const int64_t wi = e / per, r = e % per;
    const int32_t u = rep[wi * K + r / slot_words];
    out[e] = u >= 0 ? pick[(wi * nsm + u) * slot_words + r % slot_words] : 0.0;
}

// the quantile arguments of mr_windows_timeline_q, and what a chunk's quantile work keeps until its read-back
struct TlQuant {
    const double* q;
    int32_t n_q;
    int method;
    double* out;   // tl_q (host)
};
struct TlqScratch {
    DBuf<int64_t> words, off, endp, count;
    DBuf<uint64_t> key;
    DBuf<double> pick;
    SortScratch sort;
};

// The quantiles of a chunk of cw windows (dw, drep: its descriptors and answering slots; rb, tb: k_tl_count's
// grid) into out [cw * K * B * 2 * n_q] (device, zeroed).  One sizing read-back; everything else is enqueued.
int tlq_chunk(mr_ctx* ctx, const char* who, const TlWin* dw, const int32_t* drep, int32_t cw, int64_t rb, int64_t tb,
              int32_t K, int32_t B, int32_t nsm, const TlQuant& Q, const double* dq, TlqScratch& ws, double* out) {
    hipStream_t st = ctx->stream;
    const dim3 grid((unsigned)(rb + tb), (unsigned)cw);
    const int64_t init[3] = {0, INT64_MAX, INT64_MIN};
    MR_TRY(ws.words.upload(ctx, init, 3));
    hipLaunchKernelGGL(k_tlq_select<false>, grid, dim3(TL_T), 0, st, dw, (int32_t)rb, B, nsm, 0ll, 0,
                       (unsigned long long*)ws.words.p, (uint64_t*)nullptr, (int64_t)0);
    MR_TRY_HIP(ctx, hipGetLastError());
    int64_t h[3];
    MR_TRY(mr_read_words(ctx, ws.words.p, 3, h));   // (syncs)
    const int64_t total = h[0];
    if (total == 0) return MR_OK;   // every class is empty: the zeros stay
    const int64_t vmin = h[1];
    const int64_t NC = (int64_t)cw * nsm * B * 2;
    const int cb = bits_for((uint64_t)(NC - 1)), db = bits_for((uint64_t)h[2] - (uint64_t)h[1]);
    if (cb + db > 64)
        return mr_fail(ctx, MR_ERR_ARG,
                       "%s: value range too wide to sort (%lld .. %lld needs %d bits beside %d class bits; 64 in all)", who,
                       (long long)h[1], (long long)h[2], db, cb);
    const int64_t NQ = NC * Q.n_q;
    MR_TRY(ws.key.alloc(ctx, (size_t)total));
    MR_TRY(ws.off.zero(ctx, (size_t)NC));
    MR_TRY(ws.endp.zero(ctx, (size_t)NC));
    MR_TRY(ws.pick.alloc(ctx, (size_t)NQ));
    MR_TRY(ws.count.alloc(ctx, (size_t)NC));
    MR_TRY_HIP(ctx, hipMemsetAsync(ws.words.p, 0, sizeof(int64_t), st));   // the append cursor
    hipLaunchKernelGGL(k_tlq_select<true>, grid, dim3(TL_T), 0, st, dw, (int32_t)rb, B, nsm, (long long)vmin, db,
                       (unsigned long long*)ws.words.p, ws.key.p, total);
    MR_TRY(mr_radix_sort(ctx, ws.key.p, nullptr, total, cb + db, ws.sort));
    hipLaunchKernelGGL(k_tlq_bounds, dim3(cdiv(total, TL_T)), dim3(TL_T), 0, st, ws.key.p, total, db, ws.off.p, ws.endp.p);
    hipLaunchKernelGGL(k_tlq_pick, dim3(cdiv(NQ, TL_T)), dim3(TL_T), 0, st, ws.key.p, ws.off.p, ws.endp.p, NC, dq, Q.n_q,
                       Q.method, vmin, db, ws.pick.p, ws.count.p);
    const int64_t n = (int64_t)cw * K * B * 2 * Q.n_q;
    hipLaunchKernelGGL(k_tlq_gather, dim3(cdiv(n, TL_T)), dim3(TL_T), 0, st, drep, (const double*)ws.pick.p, K, B, nsm,
                       Q.n_q, n, out);
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;
}

// both entries: Q == nullptr is mr_windows_timeline, launch for launch
int tl_run(mr_ctx* ctx, const char* who, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
           const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid, const int32_t* podops,
           const int32_t* n_ops, int32_t K, int what, const int64_t* b0, const int64_t* bw, int32_t B, const TlQuant* Q,
           int64_t* tl_cnt, int64_t* tl_sum, int64_t* tl_max, int64_t* tl_out, int32_t* status) {
    const EvList L{n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K};
    MR_TRY(ev_check_args(ctx, who, L,
                         (!Q || Q->q) && (!n_windows || (b0 && bw && tl_cnt && tl_sum && tl_max && tl_out && status && (!Q || Q->out))),
                         TL_MAXOPS));
    if (B < 1 || B > TL_MAXB) return mr_fail(ctx, MR_ERR_ARG, "%s: B = %d is not in 1..%d", who, B, TL_MAXB);
    if (what != MR_LAT_DURATION && what != MR_LAT_SELF) return mr_fail(ctx, MR_ERR_ARG, "%s: unknown what %d", who, what);
    if (Q) MR_TRY(lat_args(ctx, who, what, Q->q, Q->n_q, Q->method));
    MR_TRY(ev_check_windows(ctx, who, L, true, [&](int32_t i) {
        return bw[i] > 0 ? MR_OK
                         : mr_fail(ctx, MR_ERR_ARG, "%s: window %d: the bucket width %lld is not positive", who, i, (long long)bw[i]);
    }));
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        bool all = false;
        for (int32_t j = 0; j < n_ops[i]; ++j) all = all || podops[(size_t)i * K + j] < 0;
        if (!s->has_times)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no startTime/endTime columns (a bucket is a "
                           "range of trace starts)", who, i);
        // (an unindexed table with rows has no trace-level times on record: its traces' starts were never compared)
        if (s->indexed ? !s->uniform_times : s->S > 0)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no trace-level times (a trace must fall in one "
                           "bucket)", who, i);
        if (what == MR_LAT_SELF && s->grow.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: self time on a trace shard of a larger table (children may lie "
                           "on another rank)", who, i);
        if (all && s->grow.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: slot -1 on a trace shard of a larger table (its counts would "
                           "cover this rank's traces only)", who, i);
        if (all && !s->indexed)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: slot -1 on a table without the per-trace index (it is empty, "
                           "or its key bits did not fit)", who, i);
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (n_windows == 0) return MR_OK;
    const size_t R1 = (size_t)K * B * 2, R2 = (size_t)K * 4;   // output words of a window
    for (int64_t* p : {tl_cnt, tl_sum, tl_max}) std::fill(p, p + (size_t)n_windows * R1, (int64_t)0);
    std::fill(tl_out, tl_out + (size_t)n_windows * R2, (int64_t)0);
    std::fill(status, status + n_windows, (int32_t)MR_OK);
    const size_t RQ = Q ? R1 * (size_t)Q->n_q : 0;   // tl_q words of a window
    if (Q) std::fill(Q->out, Q->out + (size_t)n_windows * RQ, 0.0);
    hipStream_t st = ctx->stream;
    const int forced_chunk = knob_int("MR_TL_CHUNK"), forced_blocks = knob_int("MR_TL_BLOCKS");
    const int32_t BB = B + 2;
    const size_t wds = (size_t)K * BB * 2 * 3;   // dense counter words of a window
    EvSlos slos;
    DBuf<double> dq;
    if (Q) MR_TRY(dq.upload(ctx, Q->q, (size_t)Q->n_q));
    for (int32_t c0 = 0; c0 < n_windows;) {
        size_t words = 0;   // (the cut counts the chunk's tl_q words too)
        const int32_t c1 = ev_chunk_end(c0, n_windows, forced_chunk, 8, [&](int32_t) { return wds + RQ; }, &words);
        const int32_t cw = c1 - c0;
        words = (size_t)cw * wds;
        const size_t n1 = (size_t)cw * R1, n2 = (size_t)cw * R2, nq = (size_t)cw * RQ;
        TlqScratch qs;
        std::vector<DBuf<uint8_t>> dstate((size_t)cw);
        std::vector<TlWin> hw((size_t)cw);
        std::vector<int32_t> rep((size_t)cw * K, -1);   // the slot that answers asked entry j (a duplicate: its first appearance's)
        DBuf<unsigned long long> cnt, ob;
        MR_TRY(cnt.zero(ctx, words));
        // ob, the chunk's ONE read-back: [cw * DW] the detectors' counter shards (u64), then as int64 [n1] counts,
        // [n1] sums, [n1] maxima, [n2] the outside counts; then as double [nq] the quantiles (mr_windows_timeline_q)
        constexpr size_t DW = EV_DW;
        const size_t ob_words = (size_t)cw * DW + 3 * n1 + n2 + nq;
        MR_TRY(ob.zero(ctx, ob_words));
        std::vector<char> det_async((size_t)cw, 0);
        int32_t n_async = 0, n_asked = 0, nsm = 0;   // nsm: the most distinct slots of a window
        int64_t maxS = 0, maxNT = 0;
        for (int32_t i = 0; i < cw; ++i) {
            const int32_t gi = c0 + i;
            const mr_spans* s = spans[gi];
            const int32_t NT = s->n_traces;
            // (a table without rows goes through the row-level detector)
            bool launched = false, empty = false;
            MR_TRY(ev_partition(ctx, L, gi, slos, dstate[(size_t)i], ob.p + (size_t)i * DW, &launched, &empty, status));
            det_async[(size_t)i] = launched;
            n_async += launched;
            TlWin& w = hw[(size_t)i];
            memset(&w, 0, sizeof w);
            w.podop = s->podop.p;
            w.trace = s->trace.p;
            w.dur = s->duration.p;
            w.span = s->span.p;
            w.tts = s->tts.p;
            w.tte = s->tte.p;
            w.state = dstate[(size_t)i].p;
            w.cnt = cnt.p + (size_t)i * wds;
            w.n_codes = s->n_span_codes;
            w.b0 = (long long)b0[gi];
            w.bw = (unsigned long long)bw[gi];
            w.NT = NT;
            w.all_slot = -1;
            if (!(empty || NT == 0 || s->S == 0 || !s->indexed))
                ev_slots(podops + (size_t)gi * K, n_ops[gi], w.op, &w.n_ops, &w.all_slot, &rep[(size_t)i * K]);
            w.direct = (int64_t)w.n_ops * BB * 2 <= EV_H;
            if (w.n_ops - (w.all_slot >= 0)) {   // (a pod-op is asked)
                if (what == MR_LAT_SELF) {
                    MR_TRY(lat_csum_ensure(ctx, s));
                    w.csum = s->csum.p;
                }
                w.S = s->S;
                maxS = std::max<int64_t>(maxS, s->S);
            }
            if (w.all_slot >= 0) {
                w.NTp = NT;
                maxNT = std::max<int64_t>(maxNT, NT);
            }
            n_asked += w.n_ops;
            nsm = std::max(nsm, w.n_ops);
        }
        DBuf<TlWin> dw;
        DBuf<int32_t> drep;
        if (n_asked > 0) {
            MR_TRY(dw.upload(ctx, hw.data(), (size_t)cw));   // (hw and rep live until the read-back's sync below)
            MR_TRY(drep.upload(ctx, rep.data(), rep.size()));
            // a block keeps its counters in LDS over all its tiles and adds them to the window's once: few
            // blocks per window where the chunk's windows fill the device anyway
            const int64_t rtiles = cdiv(maxS, TL_TILE), ttiles = cdiv(maxNT, TL_TILE);
            const int64_t per = ev_block_cap(8, cw);
            const int64_t rb = forced_blocks ? std::min<int64_t>(forced_blocks, rtiles)
                                             : std::min<int64_t>(rtiles, std::min<int64_t>(TL_MAX_CB, per));
            const int64_t tb = forced_blocks ? std::min<int64_t>(forced_blocks, ttiles)
                                             : std::min<int64_t>(ttiles, std::max<int64_t>(1, per / 4));
            if (rb + tb > 0)
                hipLaunchKernelGGL(k_tl_count, dim3((unsigned)(rb + tb), (unsigned)cw), dim3(TL_T), 0, st, (const TlWin*)dw.p,
                                   (int32_t)rb, B);
            long long* oc = (long long*)(ob.p + (size_t)cw * DW);
            hipLaunchKernelGGL(k_tl_finish, dim3((unsigned)cdiv((int64_t)(n1 + n2), TL_T)), dim3(TL_T), 0, st,
                               (const TlWin*)dw.p, (const int32_t*)drep.p, K, B, (int64_t)n1, (int64_t)n2, oc, oc + n1,
                               oc + 2 * n1, oc + 3 * n1);
            MR_TRY_HIP(ctx, hipGetLastError());
            if (Q && rb + tb > 0)
                MR_TRY(tlq_chunk(ctx, who, dw.p, drep.p, cw, rb, tb, K, B, nsm, *Q, dq.p, qs, (double*)(oc + 3 * n1 + n2)));
        }
        if (n_asked > 0 || n_async > 0) {
            MR_TRY(mr_pin_ex(ctx, ob.p, ob_words, who));
            ev_launched_status(ctx->pin_ex, det_async, c0, status);
            if (n_asked > 0) {
                const int64_t* h = (const int64_t*)(ctx->pin_ex + (size_t)cw * DW);
                memcpy(tl_cnt + (size_t)c0 * R1, h, n1 * sizeof(int64_t));
                memcpy(tl_sum + (size_t)c0 * R1, h + n1, n1 * sizeof(int64_t));
                memcpy(tl_max + (size_t)c0 * R1, h + 2 * n1, n1 * sizeof(int64_t));
                memcpy(tl_out + (size_t)c0 * R2, h + 3 * n1, n2 * sizeof(int64_t));
                if (Q) memcpy(Q->out + (size_t)c0 * RQ, h + 3 * n1 + n2, nq * sizeof(double));
            }
        }
        c0 = c1;
    }
    return MR_OK;   // (every chunk ended in a synchronise: the pinned read-back, or a row-level detector's size read-back)
}
}  // namespace

extern "C" int mr_windows_timeline(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                   const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                   const int32_t* podops, const int32_t* n_ops, int32_t K, int what, const int64_t* b0,
                                   const int64_t* bw, int32_t B, int64_t* tl_cnt, int64_t* tl_sum, int64_t* tl_max,
                                   int64_t* tl_out, int32_t* status) {
    return tl_run(ctx, "mr_windows_timeline", n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K, what, b0, bw, B,
                  nullptr, tl_cnt, tl_sum, tl_max, tl_out, status);
}

extern "C" int mr_windows_timeline_q(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                     const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                     const int32_t* podops, const int32_t* n_ops, int32_t K, int what, const int64_t* b0,
                                     const int64_t* bw, int32_t B, const double* q, int32_t n_q, int method,
                                     int64_t* tl_cnt, int64_t* tl_sum, int64_t* tl_max, int64_t* tl_out, double* tl_q,
                                     int32_t* status) {
    const TlQuant Q{q, n_q, method, tl_q};
    return tl_run(ctx, "mr_windows_timeline_q", n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K, what, b0, bw, B,
                  &Q, tl_cnt, tl_sum, tl_max, tl_out, status);
}
