// What the evidence entries over a list of windows share (mr_windows_latency, _kind_breakdown, _call_edges,
// _timeline, _replicas, _endpoints; the list pieces also serve mr_exemplar.hip).  Host: the checks of the nine
// leading arguments, the call's SLO uploads, a window's detector partition, the asked codes' slots, the chunk
// cut, the list-block plan and the one pinned read-back.  Device: the block's counter table in LDS that
// k_ce_count, k_tl_count, k_rp_count and k_ep_count keep, and the selection of a slot's first m live entries
// that k_rp_select and k_ep_select run.  An entry keeps what differs for a reason: its own requirements of a
// table (MR_ERR_STATE), its device descriptor, its kernels, its read-back layout and its scatter loop.
#pragma once
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "mr_prim.h"

// ---------------------------------------------------------------- the window list
// the nine leading arguments of an entry (include/microrank_hip.h)
struct EvList {
    int32_t n;
    const mr_spans* const* spans;
    const int64_t *t0, *t1;
    const double* const* a3;
    const uint8_t* const* a3_valid;
    const int32_t *podops, *n_ops;   // [n * K] asked codes, [n] how many of them count
    int32_t K;
};

// The list's pointers (own_ok: the entry's own are there too) and K in 1..kmax
inline int ev_check_args(mr_ctx* ctx, const char* who, const EvList& a, bool own_ok, int32_t kmax) {
    if (!ctx || a.n < 0 || !own_ok || (a.n && (!a.spans || !a.t0 || !a.t1 || !a.a3 || !a.a3_valid || !a.podops || !a.n_ops)))
        return mr_fail(ctx, MR_ERR_ARG, "%s: bad arguments", who);
    if (a.K < 1 || a.K > kmax) return mr_fail(ctx, MR_ERR_ARG, "%s: K = %d is not in 1..%d", who, a.K, kmax);
    return MR_OK;
}
inline int ev_no_check(int32_t) { return MR_OK; }
// ... then window by window: its table is the context's and its SLO arrays are there, own(i) (the entry's
// own arguments of window i), n_ops in 0..K, every asked code a pod-op code of the table (or -1: allow_all)
template <class Own = int (*)(int32_t)>
int ev_check_windows(mr_ctx* ctx, const char* who, const EvList& a, bool allow_all, Own own = ev_no_check) {
    for (int32_t i = 0; i < a.n; ++i) {
        const mr_spans* s = a.spans[i];
        if (!s || s->ctx != ctx || !a.a3[i] || !a.a3_valid[i]) return mr_fail(ctx, MR_ERR_ARG, "%s: bad window %d", who, i);
        MR_TRY(own(i));
        if (a.n_ops[i] < 0 || a.n_ops[i] > a.K)
            return mr_fail(ctx, MR_ERR_ARG, "%s: n_ops[%d] = %d is not in 0..%d", who, i, a.n_ops[i], a.K);
        for (int32_t j = 0; j < a.n_ops[i]; ++j) {
            const int32_t c = a.podops[(size_t)i * a.K + j];
            if (c < (allow_all ? -1 : 0) || c >= s->n_podops)
                return mr_fail(ctx, MR_ERR_ARG, "%s: window %d: podops[%d] = %d is %s pod-op code of the table (%d)", who, i, j,
                               c, allow_all ? "neither -1 nor a" : "no", s->n_podops);
        }
    }
    return MR_OK;
}

// ---------------------------------------------------------------- a window's partition
// Windows that give the same SLO arrays for the same number of ops share one upload (the call's).
struct EvSlos {
    struct Slo {
        DBuf<double> a3;
        DBuf<uint8_t> ok;
    };
    std::map<std::tuple<const double*, const uint8_t*, int32_t>, Slo> by_arrays;
    int get(mr_ctx* ctx, const EvList& a, int32_t i, const Slo** out) {
        const int32_t n = a.spans[i]->n_svcops;
        Slo& sl = by_arrays[std::make_tuple(a.a3[i], a.a3_valid[i], n)];
        if (!sl.a3.p) {
            MR_TRY(sl.a3.upload(ctx, a.a3[i], (size_t)n));
            MR_TRY(sl.ok.upload(ctx, a.a3_valid[i], (size_t)n));
        }
        *out = &sl;
        return MR_OK;
    }
};

constexpr size_t EV_DW = 3 * MR_DETECT_SHARDS;   // counter words of a launched detector

// Window i's partition into state (zeroed here; 0 / 1 / 2 per trace).  With counts -- EV_DW zeroed device
// words of the caller's read-back -- and a table indexed with trace-level times, the per-trace detector is
// launched only (*launched): an empty window's states stay 0, its kernels answer the padding, and
// ev_launched_status finds it after the read-back.  Else mr_detect_dev, which reads its sizes back:
// *empty, with status[i] = MR_ERR_VALUE, for a window that holds no row (T2: "Current span list is empty").
inline int ev_partition(mr_ctx* ctx, const EvList& a, int32_t i, EvSlos& slos, DBuf<uint8_t>& state,
                        unsigned long long* counts, bool* launched, bool* empty, int32_t* status) {
    const mr_spans* s = a.spans[i];
    const EvSlos::Slo* sl = nullptr;
    MR_TRY(slos.get(ctx, a, i, &sl));
    MR_TRY(state.zero(ctx, (size_t)std::max(s->n_traces, 1)));
    *launched = counts && s->indexed && s->uniform_times;
    *empty = false;
    if (*launched) return mr_detect_indexed_launch(ctx, s, a.t0[i], a.t1[i], sl->a3.p, sl->ok.p, state.p, counts);
    int32_t na = 0, nn = 0;
    int64_t nin = 0;
    const int rc = mr_detect_dev(ctx, s, a.t0[i], a.t1[i], sl->a3.p, sl->ok.p, state.p, &na, &nn, &nin);
    *empty = rc == MR_ERR_VALUE && nin == 0;
    if (*empty) status[i] = MR_ERR_VALUE;
    return *empty ? MR_OK : rc;
}
// the launched detectors of a chunk [c0, c0 + launched.size()) after its read-back: words, the pinned
// counts (EV_DW per window of the chunk)
inline void ev_launched_status(const unsigned long long* words, const std::vector<char>& launched, int32_t c0, int32_t* status) {
    for (size_t i = 0; i < launched.size(); ++i) {
        if (!launched[i]) continue;
        int32_t na = 0, nn = 0;
        int64_t nin = 0;
        mr_detect_sum(words + i * EV_DW, &na, &nn, &nin);
        if (nin == 0) status[c0 + (int32_t)i] = MR_ERR_VALUE;   // T2: "Current span list is empty"
    }
}

// ---------------------------------------------------------------- asked codes, chunks, blocks, read-back
// A window's distinct asked codes take the slots of their first appearance: op[0, *n_slots) the codes by slot,
// rep[j] the slot that answers asked entry j (a duplicate: its first appearance's), *all_slot (where given)
// the slot of -1, or -1: not asked.  *n_slots starts at 0.
inline void ev_slots(const int32_t* asked, int32_t n_asked, int32_t* op, int32_t* n_slots, int32_t* all_slot, int32_t* rep) {
    if (all_slot) *all_slot = -1;
    for (int32_t j = 0; j < n_asked; ++j) {
        int32_t u = 0;
        while (u < *n_slots && op[u] != asked[j]) ++u;
        if (u == *n_slots) {
            op[(*n_slots)++] = asked[j];
            if (all_slot && asked[j] < 0) *all_slot = u;
        }
        rep[j] = u;
    }
}

constexpr size_t EV_SCRATCH_BYTES = (size_t)64 << 20;   // a chunk's dense counters
constexpr int EV_MAX_Y = 32768;                         // windows per launch (gridDim.y)
// The chunk from window c0: consecutive windows while their dense counters (words(i) words of word_bytes
// each) fit EV_SCRATCH_BYTES -- at least one, at most EV_MAX_Y -- or `forced` of them (the entry's
// MR_xx_CHUNK).  Returns the chunk's end; *total: its words.
template <class Words>
int32_t ev_chunk_end(int32_t c0, int32_t n, int forced, size_t word_bytes, Words words, size_t* total) {
    int32_t c1 = c0;
    *total = 0;
    while (c1 < n && c1 - c0 < EV_MAX_Y) {
        const size_t wds = words(c1);
        if (forced ? c1 - c0 >= forced : (c1 > c0 && (*total + wds) * word_bytes > EV_SCRATCH_BYTES)) break;
        *total += wds;
        ++c1;
    }
    return c1;
}

// The blocks that select a launch's lists, a share per window: `want` blocks for a window's `items` items,
// at most cap (its share of the device) and max_nb (what one merge takes), or `forced` of them (the
// entry's MR_xx_BLOCKS).  Blocks [b0, b0 + nb) of the launch's lists are the window's, `per` items each.
struct EvBlocks {
    int forced;
    int64_t cap, max_nb;
    int64_t nblk = 0, widest = 0;   // blocks of the launch so far; the most of one window
    // live: the window takes part in the launch (else its nb / per still describe an empty walk)
    template <class Per>
    void add(int64_t items, int64_t want, bool live, int32_t* nb, Per* per, int32_t* b0) {
        const int64_t b = std::max<int64_t>(1, std::min<int64_t>(forced ? forced : std::min(want, cap), max_nb));
        *nb = (int32_t)b;
        *per = (Per)((std::max<int64_t>(items, 1) + b - 1) / b);
        *b0 = (int32_t)nblk;
        if (live) {
            nblk += b;
            widest = std::max(widest, b);
        }
    }
};
inline int64_t ev_block_cap(int per_cu, int64_t windows) { return std::max<int64_t>(1, (int64_t)per_cu * num_cus() / windows); }

// `words` device words into the context's pinned read-back words (ctx->pin_ex, grown to hold them); syncs
// the stream
inline int mr_pin_ex(mr_ctx* ctx, const unsigned long long* dev, size_t words, const char* who) {
    if (ctx->pin_ex_n < words) {
        if (ctx->pin_ex) (void)hipHostFree(ctx->pin_ex);
        ctx->pin_ex = nullptr;
        ctx->pin_ex_n = 0;
        if (hipHostMalloc((void**)&ctx->pin_ex, words * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
            return mr_fail(ctx, MR_ERR_OOM, "%s: pinned read-back words", who);
        ctx->pin_ex_n = words;
    }
    MR_TRY_HIP(ctx, hipMemcpyAsync(ctx->pin_ex, dev, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MR_OK;
}

// ---------------------------------------------------------------- the block's counter table (device)
// (n, sum, biased max) of the values of one key: a maximum travels as v ^ 2^63 -- order-preserving as an
// unsigned value, and the zeroed counter is the smallest; sums are uint64 (int64 sums that wrap, whatever
// the order).  wave_run_reduce's payload.
constexpr unsigned long long EV_BIAS = 1ull << 63;
struct EvRun {
    unsigned long long n, sum, mx;
    __device__ __forceinline__ EvRun up(int off) const {
        return EvRun{__shfl_up(n, off, WAVE), __shfl_up(sum, off, WAVE), __shfl_up(mx, off, WAVE)};
    }
    __device__ __forceinline__ void merge(const EvRun& lower) {
        n += lower.n;
        sum += lower.sum;
        mx = lower.mx > mx ? lower.mx : mx;
    }
};
// a lane's own value d (has: the lane brings one)
__device__ __forceinline__ EvRun ev_run_of(bool has, unsigned long long d) {
    return EvRun{has ? 1ull : 0ull, has ? d : 0ull, has ? d ^ EV_BIAS : 0ull};
}
// the dense global counters: three words per key
template <class K>
__device__ __forceinline__ void ev_add(unsigned long long* cnt, K kd, const EvRun& r) {
    unsigned long long* p = cnt + (size_t)kd * 3;
    atomicAdd(p, r.n);
    atomicAdd(p + 1, r.sum);
    atomicMax(p + 2, r.mx);
}
// A block works through many tiles and keeps EV_H keys' counters in LDS (32 KB), adding them to the global
// counters once, at its end: a few thousand hot addresses would otherwise take three global atomics per
// run of a few rows.  direct: the keys are below EV_H and entry kd is key kd's (k is unused).  Else the
// slot of kd's hash, claimed by the first key that comes (k holds key + 1; 0: free); a key that finds its
// slot taken by another adds to the global counters itself.  Integer adds and maxima either way: the
// same bits, whatever the cut and whichever path a run took.
constexpr int EV_HB = 10, EV_H = 1 << EV_HB;
struct EvTable {
    unsigned long long k[EV_H], n[EV_H], s[EV_H], m[EV_H];
    // (a barrier between clear, the adds and flush is the caller's)
    __device__ __forceinline__ void clear(int tid, int threads) {
        for (int i = tid; i < EV_H; i += threads) k[i] = n[i] = s[i] = m[i] = 0ull;
    }
    template <class K>
    __device__ __forceinline__ void add(bool direct, unsigned long long* cnt, K kd, const EvRun& r) {
        uint32_t h = (uint32_t)kd;
        if (!direct) {
            h = (uint32_t)(((unsigned long long)kd * 0x9E3779B97F4A7C15ull) >> (64 - EV_HB));
            const unsigned long long mine = (unsigned long long)kd + 1ull;
            const unsigned long long prev = atomicCAS(&k[h], 0ull, mine);
            if (prev != 0ull && prev != mine) {
                ev_add(cnt, kd, r);
                return;
            }
        }
        atomicAdd(&n[h], r.n);
        atomicAdd(&s[h], r.sum);
        atomicMax(&m[h], r.mx);
    }
    template <class K>
    __device__ __forceinline__ void flush(bool direct, unsigned long long* cnt, int tid, int threads) {
        for (int i = tid; i < EV_H; i += threads)
            if (direct ? n[i] != 0ull : k[i] != 0ull) ev_add(cnt, direct ? (K)i : (K)(k[i] - 1ull), EvRun{n[i], s[i], m[i]});
    }
};

// ---------------------------------------------------------------- a slot's selection (device)
// What k_rp_select (mr_replicas.hip) and k_ep_select (mr_endpoints.hip) share: a slot's R dense counters of six
// words -- side 0's {n, sum, biased max}, then side 1's -- its live count, its totals, and the first m live
// entries under the order (abnormal count descending, normal count ascending, place q ascending).
// A live entry's place in the order; q < 0: none
struct EvKey {
    unsigned long long ca, cn;
    int32_t q;
};
__device__ __forceinline__ bool ev_before(const EvKey& a, const EvKey& b) {
    return a.ca != b.ca ? a.ca > b.ca : a.cn != b.cn ? a.cn < b.cn : a.q < b.q;
}
__device__ __forceinline__ EvKey ev_better(const EvKey a, const EvKey b) {
    const bool pa = b.q < 0 || (a.q >= 0 && ev_before(a, b));   // (field by field: selects, no addresses)
    return EvKey{pa ? a.ca : b.ca, pa ? a.cn : b.cn, pa ? a.q : b.q};
}
// a counter's maximum as the answer gives it: un-biased, 0 where the count is 0
__device__ __forceinline__ unsigned long long ev_max_of(unsigned long long n, unsigned long long mx) {
    return n ? mx ^ EV_BIAS : 0ull;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long x = __shfl_xor(v, o, WAVE);
        v = x > v ? x : v;
    }
    return v;
}
constexpr int EV_SW = 8;   // a selection record: live, n, tot[2][3], then m entries of 7 words
// A block of T threads (every thread calls it) selects over c[R * 6]: rec[0] live, rec[1] n = min(m, live),
// rec[2 .. 8) the totals (side, {cnt, sum, max}), then n entries of 7 words: code_of(q), its (cnt, sum, max) on
// side 0 and on side 1.  The live count, the totals, then m rounds of a block-wide best-of-rest; the two counts
// are compared as they are -- no packed key -- so the order is exact for any count.  tot[7] and wbest[T / WAVE]
// are the block's shared words.
template <int T, class CodeOf>
__device__ __forceinline__ void ev_select_block(const unsigned long long* __restrict__ c, int32_t R,
                                                unsigned long long* __restrict__ rec, int32_t m, CodeOf code_of,
                                                unsigned long long* tot, EvKey* wbest) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if (threadIdx.x < 7) tot[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long lv = 0ull, c0 = 0ull, s0 = 0ull, x0 = 0ull, c1 = 0ull, s1 = 0ull, x1 = 0ull;   // live; {cnt, sum, biased max} of side 0, 1
    for (int32_t q = (int32_t)threadIdx.x; q < R; q += T) {
        const unsigned long long* p = c + (size_t)q * 6;
        lv += p[0] + p[3] > 0ull;
        c0 += p[0];
        s0 += p[1];
        x0 = p[2] > x0 ? p[2] : x0;
        c1 += p[3];
        s1 += p[4];
        x1 = p[5] > x1 ? p[5] : x1;
    }
    lv = wave_sum_u64(lv);
    c0 = wave_sum_u64(c0);
    s0 = wave_sum_u64(s0);
    x0 = wave_max_u64(x0);
    c1 = wave_sum_u64(c1);
    s1 = wave_sum_u64(s1);
    x1 = wave_max_u64(x1);
    if (lane == 0) {
        atomicAdd(&tot[0], lv);
        atomicAdd(&tot[1], c0);
        atomicAdd(&tot[2], s0);
        atomicMax(&tot[3], x0);
        atomicAdd(&tot[4], c1);
        atomicAdd(&tot[5], s1);
        atomicMax(&tot[6], x1);
    }
    __syncthreads();
    const unsigned long long live = tot[0];
    const int32_t n = (int32_t)(live < (unsigned long long)m ? live : (unsigned long long)m);
    if (threadIdx.x == 0) {
        rec[0] = live;
        rec[1] = (unsigned long long)n;
        rec[2] = tot[1];
        rec[3] = tot[2];
        rec[4] = ev_max_of(tot[1], tot[3]);
        rec[5] = tot[4];
        rec[6] = tot[5];
        rec[7] = ev_max_of(tot[4], tot[6]);
    }
    EvKey last{0ull, 0ull, -1};
    for (int32_t e = 0; e < n; ++e) {   // (block-uniform: n <= live, so every round finds an entry)
        EvKey best{0ull, 0ull, -1};
        for (int32_t q = (int32_t)threadIdx.x; q < R; q += T) {
            const EvKey k{c[(size_t)q * 6 + 3], c[(size_t)q * 6], q};
            if (k.ca + k.cn == 0ull) continue;
            if (last.q >= 0 && !ev_before(last, k)) continue;   // (listed already)
            best = ev_better(best, k);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const EvKey x{__shfl_xor(best.ca, o, WAVE), __shfl_xor(best.cn, o, WAVE), __shfl_xor(best.q, o, WAVE)};
            best = ev_better(best, x);
        }
        __syncthreads();   // (the round before has read wbest)
        if (lane == 0) wbest[wv] = best;
        __syncthreads();
        best = wbest[0];
#pragma unroll
        for (int i = 1; i < T / WAVE; ++i) best = ev_better(best, wbest[i]);
        last = best;
        if (threadIdx.x == 0 && best.q >= 0) {
            const unsigned long long* p = c + (size_t)best.q * 6;
            unsigned long long* o = rec + EV_SW + (size_t)e * 7;
            o[0] = (unsigned long long)(long long)code_of(best.q);
            o[1] = p[0];
            o[2] = p[1];
            o[3] = ev_max_of(p[0], p[2]);
            o[4] = p[3];
            o[5] = p[4];
            o[6] = ev_max_of(p[3], p[5]);
        }
    }
}
