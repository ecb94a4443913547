// Replica evidence of a window (no reference counterpart): per asked pod-op, the pod-ops that share its
// service-op -- its replicas -- with the count, summed value and largest value of their rows on the normal
// and on the abnormal side of the window's own detector partition.  The other evidence entries describe the
// asked pod-op in isolation; this one says whether it is the POD (its siblings are fine) or the OPERATION
// (every replica is slow on the abnormal traces).  It is the first entry that reads svcop on the evidence
// path, and it keeps one small index per table:
//   the replica index (rp_index_ensure, once per table, kept on the mr_spans like csum):
//   k_rp_map     a lane per row: integer atomicMin / atomicMax of svcop into po_lo[podop] / po_hi[podop]
//                (order-free); k_rp_keys then counts the pod-ops with two service-ops (an ambiguous table is
//                refused, its verdict kept) and writes (sv, code) pairs; ONE stable mr_radix_sort by sv groups
//                the pod-ops with rows in code order; k_rp_group / k_rp_rank leave rp_off[n_svcops + 1],
//                rp_pods[] and rp_rank[p], the place of p inside its group
//   k_rp_count   one launch for a chunk's windows (gridDim.y), k_tl_count's row pass: a lane per row, RP_U
//                rows in flight per lane: the row's trace state first (a row outside the partition reads
//                nothing more; reading the service-op first instead was measured and is no faster: DESIGN
//                §3), then its service-op and that code's slot among the window's distinct asked
//                SERVICE-ops (at most 64, in LDS, behind a 64-bit filter of code & 63 in registers), then
//                its pod-op and rp_rank, then the value -- for MR_LAT_SELF span and csum, read only by rows
//                that have a slot.  key = (base[slot] + rank) * 2 + side; runs of equal keys inside a wave are
//                reduced (mr_prim.h wave_run_reduce) and the run's last lane adds n, the sum and the maximum
//                to the block's counter table in LDS (mr_evidence.h EvTable), direct-mapped where the window's
//                keys fit, else hashed.  The block adds its table to the window's dense counters once, at
//                its end.  Slots are by service-op, so asked replicas of one operation share one set of counters
//   k_rp_select  a block per (window, distinct slot) over the slot's |R| dense counters: the live count, the
//                totals, and the first m live replicas under the order (abnormal count descending, normal
//                count ascending, code ascending) by m rounds of a block-wide best-of-rest.  The two counts
//                are compared as they are -- no packed key -- so the order is exact for any count
//   k_rp_finish  a block per (window, asked entry): the entry's planes in their final layout from its slot's
//                record (duplicates and slot-sharing entries are answered from their slot), its own numbers
//                from its counters, and its place: the live replicas ordered before it, counted by the block
// One row pass per chunk of windows -- never a launch per asked op or per replica -- and one pinned
// read-back per chunk, which carries the detectors' counts too: no host synchronisation per window.  The
// window list's front end is mr_evidence.h's; a window takes sum over its slots of |R(slot)| * 2 * 3 counter
// words plus its selection records and output planes (MR_RP_CHUNK, read per call, forces the windows per
// chunk; MR_RP_BLOCKS the row blocks per window: tests reach every cut at small sizes).
#include <climits>

#include "mr_evidence.h"
#include "mr_sort.h"

namespace {
constexpr int RP_T = 256;                     // threads per block
constexpr int RP_U = 4;                       // k_rp_count: rows in flight per lane
constexpr int RP_TILE = RP_T * RP_U;          // rows of a block's tile
constexpr int RP_MAXOPS = 64;                 // asked slots per window (the evidence entries' limit)
constexpr int RP_MAXM = 32;                   // listed replicas per asked entry
constexpr int RP_MAX_CB = 4096;               // row blocks per window (grid-stride over the tiles)
constexpr int RP_SW = EV_SW;                  // a slot's selection record (mr_evidence.h ev_select_block)
constexpr int64_t RP_MAX_KEYS = (int64_t)1 << 30;   // replicas of a window's slots: key = replica * 2 + side is an int32

struct RpWin {
    const int32_t *svcop, *podop, *trace;
    const int64_t *dur, *span;
    const int32_t *rank, *pods;           // the table's rp_rank [n_podops], rp_pods
    const unsigned long long* csum;       // nullptr: MR_LAT_DURATION
    const uint8_t* state;
    unsigned long long* cnt;              // [replicas * 2 * 3]: slot's replica, side, {n, sum, biased max}
    unsigned long long* sel;              // [n_ops * (RP_SW + 7 * m)] the slots' selection records
    int64_t S, n_codes;                   // S: the rows of the row pass (0: no slot holds a replica)
    int32_t NT, NP;                       // traces, pod-ops of the table
    int32_t n_ops, direct;                // distinct asked slots; the keys fit the block's table: direct-mapped
    int32_t op[RP_MAXOPS];                // asked service-op codes by slot (-1: the slot of pod-ops without rows)
    int32_t base[RP_MAXOPS];              // first replica of the slot among the window's
    int32_t nr[RP_MAXOPS];                // |R(slot)|
    int32_t rbeg[RP_MAXOPS];              // the slot's first entry in rp_pods
};

// ---------------------------------------------------------------- the replica index
__global__ void __launch_bounds__(RP_T) k_rp_fill(int32_t* __restrict__ lo, int32_t* __restrict__ hi,
                                                  int32_t* __restrict__ rank, int32_t n) {
    const int32_t p = (int32_t)(blockIdx.x * RP_T + threadIdx.x);
    if (p < n) {
        lo[p] = INT32_MAX;
        hi[p] = -1;
        rank[p] = -1;
    }
}
__global__ void __launch_bounds__(RP_T) k_rp_map(const int32_t* __restrict__ podop, const int32_t* __restrict__ svcop,
                                                 int64_t S, int32_t NP, int32_t NS, int32_t* __restrict__ lo,
                                                 int32_t* __restrict__ hi) {
    const int64_t r = (int64_t)blockIdx.x * RP_T + threadIdx.x;
    if (r >= S) return;
    const int32_t p = podop[r], s = svcop[r];
    if ((uint32_t)p < (uint32_t)NP && (uint32_t)s < (uint32_t)NS) {
        atomicMin(&lo[p], s);
        atomicMax(&hi[p], s);
    }
}
// bad[0]: the ambiguous pod-ops, bad[1]: the smallest of their codes.  A pod-op without rows sorts behind
// every service-op (key NS)
__global__ void __launch_bounds__(RP_T) k_rp_keys(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int32_t NP,
                                                  int32_t NS, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                  int32_t* __restrict__ bad) {
    const int32_t p = (int32_t)(blockIdx.x * RP_T + threadIdx.x);
    if (p >= NP) return;
    const bool has = hi[p] >= 0;
    if (has && lo[p] != hi[p]) {
        atomicAdd(&bad[0], 1);
        atomicMin(&bad[1], p);
    }
    keys[p] = has ? (uint64_t)lo[p] : (uint64_t)NS;
    vals[p] = (uint32_t)p;
}
// sorted position i: off[t] = i for every service-op t in (key[i - 1], key[i]]; the last position closes the rest
__global__ void __launch_bounds__(RP_T) k_rp_group(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   int32_t n, int32_t NS, int32_t* __restrict__ off,
                                                   int32_t* __restrict__ pods) {
    const int32_t i = (int32_t)(blockIdx.x * RP_T + threadIdx.x);
    if (i >= n) return;
    const uint64_t ki = keys[i], kp = i ? keys[i - 1] : 0ull;
    const int64_t s = ki < (uint64_t)NS ? (int64_t)ki : (int64_t)NS, prev = !i ? -1 : kp < (uint64_t)NS ? (int64_t)kp : (int64_t)NS;
    if (s < NS) pods[i] = (int32_t)vals[i];
    for (int64_t t = prev + 1; t <= s; ++t) off[t] = i;
    if (i == n - 1)
        for (int64_t t = s + 1; t <= NS; ++t) off[t] = n;
}
__global__ void __launch_bounds__(RP_T) k_rp_rank(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                  int32_t n, int32_t NS, const int32_t* __restrict__ off,
                                                  int32_t* __restrict__ rank) {
    const int32_t i = (int32_t)(blockIdx.x * RP_T + threadIdx.x);
    if (i >= n) return;
    const uint64_t s = keys[i];
    if (s < (uint64_t)NS && vals[i] < (uint32_t)n) rank[vals[i]] = i - off[s];
}

// the table's index, built at the first call and kept (an ambiguous table keeps its verdict only)
int rp_index_ensure(mr_ctx* ctx, const mr_spans* s) {
    if (s->rp_state) return MR_OK;
    const int32_t NP = s->n_podops, NS = s->n_svcops;
    hipStream_t st = ctx->stream;
    DBuf<int32_t> lo, hi, bad;
    DBuf<uint64_t> keys;
    DBuf<uint32_t> vals;
    SortScratch ws;
    MR_TRY(lo.alloc(ctx, (size_t)NP));
    MR_TRY(hi.alloc(ctx, (size_t)NP));
    MR_TRY(keys.alloc(ctx, (size_t)NP));
    MR_TRY(vals.alloc(ctx, (size_t)NP));
    MR_TRY(s->rp_off.zero(ctx, (size_t)NS + 1));
    MR_TRY(s->rp_pods.zero(ctx, (size_t)std::max(NP, 1)));
    MR_TRY(s->rp_rank.alloc(ctx, (size_t)std::max(NP, 1)));
    const int32_t bad0[2] = {0, INT32_MAX};
    MR_TRY(bad.upload(ctx, bad0, 2));
    std::vector<int32_t> hlo((size_t)NP), hhi((size_t)NP), off((size_t)NS + 1, 0);
    int32_t hb[2] = {0, INT32_MAX};
    if (NP > 0) {
        const unsigned nb = (unsigned)cdiv(NP, RP_T);
        hipLaunchKernelGGL(k_rp_fill, dim3(nb), dim3(RP_T), 0, st, lo.p, hi.p, s->rp_rank.p, NP);
        if (s->S > 0)
            hipLaunchKernelGGL(k_rp_map, dim3((unsigned)cdiv(s->S, RP_T)), dim3(RP_T), 0, st, (const int32_t*)s->podop.p,
                               (const int32_t*)s->svcop.p, s->S, NP, NS, lo.p, hi.p);
        hipLaunchKernelGGL(k_rp_keys, dim3(nb), dim3(RP_T), 0, st, (const int32_t*)lo.p, (const int32_t*)hi.p, NP, NS, keys.p,
                           vals.p, bad.p);
        MR_TRY_HIP(ctx, hipGetLastError());
        MR_TRY(mr_radix_sort(ctx, keys.p, vals.p, NP, bits_for((uint64_t)NS), ws));
        hipLaunchKernelGGL(k_rp_group, dim3(nb), dim3(RP_T), 0, st, (const uint64_t*)keys.p, (const uint32_t*)vals.p, NP, NS,
                           s->rp_off.p, s->rp_pods.p);
        hipLaunchKernelGGL(k_rp_rank, dim3(nb), dim3(RP_T), 0, st, (const uint64_t*)keys.p, (const uint32_t*)vals.p, NP, NS,
                           (const int32_t*)s->rp_off.p, s->rp_rank.p);
        MR_TRY_HIP(ctx, hipGetLastError());
        MR_TRY(lo.download(ctx, hlo.data(), (size_t)NP));
        MR_TRY(hi.download(ctx, hhi.data(), (size_t)NP));
    }
    MR_TRY(s->rp_off.download(ctx, off.data(), (size_t)NS + 1));
    MR_TRY(bad.download(ctx, hb, 2));
    MR_TRY_HIP(ctx, hipStreamSynchronize(st));
    s->rp_sv_h.assign((size_t)NP, -1);
    for (int32_t p = 0; p < NP; ++p)
        if (hhi[(size_t)p] >= 0) s->rp_sv_h[(size_t)p] = hlo[(size_t)p];
    s->rp_off_h.swap(off);
    if (hb[0] > 0) {
        const int32_t p = hb[1];
        s->rp_bad[0] = p;
        s->rp_bad[1] = hlo[(size_t)p];
        s->rp_bad[2] = hhi[(size_t)p];
        s->rp_off.reset();
        s->rp_pods.reset();
        s->rp_rank.reset();
        s->rp_state = 2;
    } else {
        s->rp_state = 1;
    }
    return MR_OK;
}

// ---------------------------------------------------------------- the row pass
// every lane of the wave brings (kd, d), kd < 0: nothing; runs of equal keys are reduced and added once
__device__ __forceinline__ void rp_reduce(int lane, bool direct, EvTable& tab, unsigned long long* cnt, int32_t kd,
                                          unsigned long long d) {
    if (__ballot(kd >= 0) == 0ull) return;   // (wave-uniform)
    EvRun run = ev_run_of(kd >= 0, d);
    const bool tail = wave_run_reduce(lane, kd, run);
    if (kd >= 0 && tail) tab.add(direct, cnt, kd, run);
}

__global__ void __launch_bounds__(RP_T) k_rp_count(const RpWin* __restrict__ ws) {
    __shared__ EvTable tab;   // n, sum, biased max
    __shared__ int32_t ops[RP_MAXOPS], base[RP_MAXOPS], nr[RP_MAXOPS];
    const RpWin& w = ws[blockIdx.y];
    const int64_t N = w.S;
    if ((int64_t)blockIdx.x * RP_TILE >= N) return;   // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const bool direct = w.direct != 0;
    const int32_t n_ops = w.n_ops;
    tab.clear(threadIdx.x, RP_T);
    if (threadIdx.x < RP_MAXOPS) {
        const bool in = (int)threadIdx.x < n_ops;
        ops[threadIdx.x] = in ? w.op[threadIdx.x] : -1;
        base[threadIdx.x] = in ? w.base[threadIdx.x] : 0;
        nr[threadIdx.x] = in ? w.nr[threadIdx.x] : 0;
    }
    __syncthreads();
    uint64_t filter = 0;   // bit (code & 63) of every asked service-op
    for (int j = 0; j < n_ops; ++j)
        if (ops[j] >= 0) filter |= 1ull << (ops[j] & 63);
    const uint32_t NT = (uint32_t)w.NT, NP = (uint32_t)w.NP;
    const int64_t n_codes = w.n_codes;
    const unsigned long long* __restrict__ csum = w.csum;
    for (int64_t tile = (int64_t)blockIdx.x * RP_TILE; tile < N; tile += (int64_t)gridDim.x * RP_TILE) {   // (block-uniform)
        int32_t tr[RP_U], sv[RP_U], po[RP_U], rk[RP_U];
        int st[RP_U], slot[RP_U];
#pragma unroll
        for (int k = 0; k < RP_U; ++k) {
            const int64_t c = tile + k * RP_T + threadIdx.x;
            tr[k] = c < N ? w.trace[c] : -1;
        }
#pragma unroll
        for (int k = 0; k < RP_U; ++k) st[k] = (uint32_t)tr[k] < NT ? (int)w.state[tr[k]] : 0;
#pragma unroll
        for (int k = 0; k < RP_U; ++k) {
            const int64_t c = tile + k * RP_T + threadIdx.x;
            sv[k] = st[k] == 1 || st[k] == 2 ? w.svcop[c] : -1;
        }
#pragma unroll
        for (int k = 0; k < RP_U; ++k) {
            const int64_t c = tile + k * RP_T + threadIdx.x;
            slot[k] = -1;
            if (sv[k] >= 0 && (filter >> (sv[k] & 63) & 1ull))
                for (int j = 0; j < n_ops; ++j)
                    if (ops[j] == sv[k]) slot[k] = j;   // (the asked service-ops are distinct)
            po[k] = slot[k] >= 0 ? w.podop[c] : -1;
        }
#pragma unroll
        for (int k = 0; k < RP_U; ++k) rk[k] = (uint32_t)po[k] < NP ? w.rank[po[k]] : -1;
#pragma unroll
        for (int k = 0; k < RP_U; ++k) {
            const int64_t c = tile + k * RP_T + threadIdx.x;
            int32_t kd = -1;
            unsigned long long d = 0ull;
            // (an unambiguous table puts every row of a replica inside its own group: rank < |R(slot)|)
            if (slot[k] >= 0 && (uint32_t)rk[k] < (uint32_t)nr[slot[k]]) {
                kd = (base[slot[k]] + rk[k]) * 2 + (st[k] - 1);
                d = (unsigned long long)w.dur[c];
                if (csum) {
                    const int64_t sc = w.span[c];
                    if (sc >= 0 && sc < n_codes) d -= csum[sc];
                }
            }
            rp_reduce(lane, direct, tab, w.cnt, kd, d);
        }
    }
    __syncthreads();
    tab.flush<int32_t>(direct, w.cnt, threadIdx.x, RP_T);
}

// ---------------------------------------------------------------- selection
// block (slot u, window): rec[0] live, rec[1] n = min(m, live), rec[2 .. 8) the totals (side, {cnt, sum, max}),
// then n entries of 7 words: the replica's pod-op code, its (cnt, sum, max) on side 0 and on side 1
__global__ void __launch_bounds__(RP_T) k_rp_select(const RpWin* __restrict__ ws, int32_t m) {
    __shared__ unsigned long long tot[7];
    __shared__ EvKey wbest[RP_T / WAVE];
    const RpWin& w = ws[blockIdx.y];
    const int32_t u = (int32_t)blockIdx.x;
    if (u >= w.n_ops) return;   // (block-uniform)
    const int32_t* __restrict__ pods = w.pods + w.rbeg[u];
    ev_select_block<RP_T>(w.cnt + (size_t)w.base[u] * 6, w.nr[u], w.sel + (size_t)u * (RP_SW + 7 * m), m,
                          [pods](int32_t q) { return pods[q]; }, tot, wbest);
}

// the chunk's output planes, each in the entry's final layout over the chunk's windows
struct RpOut {
    long long *cnt, *sum, *max;   // [cw * K * m * 2]
    long long *own, *tot;         // [cw * K * 6]
    int32_t* pod;                 // [cw * K * m]
    int32_t *n, *live, *all, *place;   // [cw * K]
};

// block (asked entry j, window): rep[window * K + j] the slot that answers the entry, or -1 (not asked, or a
// window without rows: the padding); asked[window * K + j] its pod-op code
__global__ void __launch_bounds__(RP_T) k_rp_finish(const RpWin* __restrict__ ws, const int32_t* __restrict__ rep,
                                                    const int32_t* __restrict__ asked, int32_t K, int32_t m, RpOut o) {
    __shared__ unsigned int before;
    const RpWin& w = ws[blockIdx.y];
    const size_t x = (size_t)blockIdx.y * K + blockIdx.x;
    const int32_t u = rep[x];
    const int32_t R = u >= 0 ? w.nr[u] : 0;
    const int32_t p = asked[x];
    const int32_t rk = R > 0 && (uint32_t)p < (uint32_t)w.NP ? w.rank[p] : -1;
    if ((uint32_t)rk >= (uint32_t)R) {   // (block-uniform) the padding; sv(p) == -1 has no replica
        for (int32_t e = (int32_t)threadIdx.x; e < m; e += RP_T) {
            o.pod[x * m + e] = -1;
            for (int sd = 0; sd < 2; ++sd) o.cnt[(x * m + e) * 2 + sd] = o.sum[(x * m + e) * 2 + sd] = o.max[(x * m + e) * 2 + sd] = 0ll;
        }
        if (threadIdx.x < 6) o.own[x * 6 + threadIdx.x] = o.tot[x * 6 + threadIdx.x] = 0ll;
        if (threadIdx.x == 0) {
            o.n[x] = o.live[x] = o.all[x] = 0;
            o.place[x] = -1;
        }
        return;
    }
    const unsigned long long* __restrict__ c = w.cnt + (size_t)w.base[u] * 6;
    const unsigned long long* __restrict__ rec = w.sel + (size_t)u * (RP_SW + 7 * m);
    const int32_t n = (int32_t)rec[1];
    for (int32_t e = (int32_t)threadIdx.x; e < m; e += RP_T) {
        const bool in = e < n;
        const unsigned long long* r = rec + RP_SW + (size_t)e * 7;
        o.pod[x * m + e] = in ? (int32_t)r[0] : -1;
        for (int sd = 0; sd < 2; ++sd) {
            o.cnt[(x * m + e) * 2 + sd] = in ? (long long)r[1 + sd * 3] : 0ll;
            o.sum[(x * m + e) * 2 + sd] = in ? (long long)r[2 + sd * 3] : 0ll;
            o.max[(x * m + e) * 2 + sd] = in ? (long long)r[3 + sd * 3] : 0ll;
        }
    }
    const unsigned long long* mine = c + (size_t)rk * 6;
    const EvKey me{mine[3], mine[0], rk};
    const bool has = me.ca + me.cn > 0ull;
    if (threadIdx.x == 0) before = 0u;
    __syncthreads();
    if (has) {   // (block-uniform)
        unsigned int b = 0;
        for (int32_t q = (int32_t)threadIdx.x; q < R; q += RP_T) {
            const EvKey k{c[(size_t)q * 6 + 3], c[(size_t)q * 6], q};
            b += k.ca + k.cn > 0ull && ev_before(k, me);
        }
        b = (unsigned int)wave_sum_u64(b);
        if ((threadIdx.x & (WAVE - 1)) == 0 && b) atomicAdd(&before, b);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int f = threadIdx.x % 3, sd = threadIdx.x / 3;
        o.own[x * 6 + threadIdx.x] = (long long)(f == 2 ? ev_max_of(mine[sd * 3], mine[sd * 3 + 2]) : mine[sd * 3 + f]);
        o.tot[x * 6 + threadIdx.x] = (long long)rec[2 + threadIdx.x];
    }
    if (threadIdx.x == 0) {
        o.n[x] = n;
        o.live[x] = (int32_t)rec[0];
        o.all[x] = R;
        o.place[x] = has ? (int32_t)before : -1;
    }
}

// The slots of a window's asked codes: the codes mapped to their service-ops (-1: a pod-op without rows),
// mr_evidence.h's ev_slots over those, then each slot's group in the table's index.  Returns the replicas
// of all the slots
int64_t rp_slots(const mr_spans* s, const int32_t* asked, int32_t n_asked, RpWin& w, int32_t* rep) {
    int32_t sva[RP_MAXOPS], none = -1;
    for (int32_t j = 0; j < n_asked; ++j) sva[j] = s->rp_sv_h[(size_t)asked[j]];
    w.n_ops = 0;
    ev_slots(sva, n_asked, w.op, &w.n_ops, &none, rep);
    int64_t total = 0;
    for (int32_t u = 0; u < w.n_ops; ++u) {
        const int32_t sv = w.op[u];
        w.rbeg[u] = sv >= 0 ? s->rp_off_h[(size_t)sv] : 0;
        w.nr[u] = sv >= 0 ? s->rp_off_h[(size_t)sv + 1] - w.rbeg[u] : 0;
        w.base[u] = (int32_t)std::min<int64_t>(total, INT32_MAX);
        total += w.nr[u];
    }
    return total;
}
}  // namespace

extern "C" int mr_windows_replicas(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                   const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                   const int32_t* podops, const int32_t* n_ops, int32_t K, int32_t m, int what,
                                   int32_t* rp_pod, int64_t* rp_cnt, int64_t* rp_sum, int64_t* rp_max, int32_t* rp_n,
                                   int32_t* rp_live, int32_t* rp_all, int32_t* rp_place, int64_t* rp_own, int64_t* rp_tot,
                                   int32_t* status) {
    const char* who = "mr_windows_replicas";
    const EvList L{n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K};
    MR_TRY(ev_check_args(ctx, who, L,
                         !n_windows || (rp_pod && rp_cnt && rp_sum && rp_max && rp_n && rp_live && rp_all && rp_place &&
                                        rp_own && rp_tot && status),
                         RP_MAXOPS));
    if (m < 1 || m > RP_MAXM) return mr_fail(ctx, MR_ERR_ARG, "%s: m = %d is not in 1..%d", who, m, RP_MAXM);
    MR_TRY(ev_check_windows(ctx, who, L, false));
    if (what != MR_LAT_DURATION && what != MR_LAT_SELF) return mr_fail(ctx, MR_ERR_ARG, "%s: unknown what %d", who, what);
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        const bool whole = t0[i] == INT64_MIN && t1[i] == INT64_MAX;
        if (!s->has_times)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no startTime/endTime columns (the window's "
                           "detector reads them, for the whole table too)", who, i);
        // (an unindexed table with rows has no trace-level times on record)
        if (!whole && (s->indexed ? !s->uniform_times : s->S > 0))
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no trace-level times (a window of it cuts traces)",
                           who, i);
        if (what == MR_LAT_SELF && s->grow.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: self time on a trace shard of a larger table (children may lie "
                           "on another rank)", who, i);
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (n_windows == 0) return MR_OK;
    {
        RpWin tmp;
        std::vector<int32_t> rep((size_t)K);
        for (int32_t i = 0; i < n_windows; ++i) {
            const mr_spans* s = spans[i];
            MR_TRY(rp_index_ensure(ctx, s));
            if (s->rp_state == 2)
                return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table is ambiguous: pod-op %d has rows of service-op %d "
                               "and of service-op %d (a pod-op's replicas are the pod-ops of ITS service-op)", who, i,
                               s->rp_bad[0], s->rp_bad[1], s->rp_bad[2]);
            const int64_t reps = rp_slots(s, podops + (size_t)i * K, n_ops[i], tmp, rep.data());
            if (reps >= RP_MAX_KEYS)
                return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: its asked service-ops hold %lld replicas; a counter's key "
                               "holds fewer than 2^30", who, i, (long long)reps);
        }
    }
    const size_t KM = (size_t)K * m;
    std::fill(rp_pod, rp_pod + (size_t)n_windows * KM, (int32_t)-1);
    for (int64_t* p : {rp_cnt, rp_sum, rp_max}) std::fill(p, p + (size_t)n_windows * KM * 2, (int64_t)0);
    for (int32_t* p : {rp_n, rp_live, rp_all}) std::fill(p, p + (size_t)n_windows * K, (int32_t)0);
    std::fill(rp_place, rp_place + (size_t)n_windows * K, (int32_t)-1);
    for (int64_t* p : {rp_own, rp_tot}) std::fill(p, p + (size_t)n_windows * K * 6, (int64_t)0);
    std::fill(status, status + n_windows, (int32_t)MR_OK);
    hipStream_t st = ctx->stream;
    const int forced_chunk = knob_int("MR_RP_CHUNK"), forced_blocks = knob_int("MR_RP_BLOCKS");
    const size_t SW = (size_t)RP_SW + 7 * (size_t)m;                       // a slot's selection record
    const size_t O64 = KM * 2 * 3 + (size_t)K * 12, O32 = KM + (size_t)K * 4;   // a window's output words, int64 and int32
    EvSlos slos;
    for (int32_t c0 = 0; c0 < n_windows;) {
        size_t words = 0;
        // a window's scratch: its dense counters, its slots' records and its output planes
        const int32_t c1 = ev_chunk_end(c0, n_windows, forced_chunk, 8, [&](int32_t i) {
            RpWin tmp;
            int32_t rep[RP_MAXOPS];
            const int64_t reps = rp_slots(spans[i], podops + (size_t)i * K, n_ops[i], tmp, rep);
            return (size_t)reps * 6 + (size_t)tmp.n_ops * SW + O64 + (O32 + 1) / 2;
        }, &words);
        const int32_t cw = c1 - c0;
        std::vector<DBuf<uint8_t>> dstate((size_t)cw);
        std::vector<RpWin> hw((size_t)cw);
        std::vector<int32_t> rep((size_t)cw * K, -1), asked((size_t)cw * K, -1);
        std::vector<size_t> cnt_at((size_t)cw, 0), sel_at((size_t)cw, 0);
        DBuf<unsigned long long> cnt, sel, ob;
        // ob, the chunk's ONE read-back: [cw * DW] the detectors' counter shards (u64), then the int64 planes
        // (counts, sums, maxima, own, totals), then the int32 planes (pods, n, live, all, place)
        constexpr size_t DW = EV_DW;
        const size_t n64 = (size_t)cw * O64, n32 = (size_t)cw * O32;
        const size_t ob_words = (size_t)cw * DW + n64 + (n32 + 1) / 2;
        MR_TRY(ob.zero(ctx, ob_words));
        std::vector<char> det_async((size_t)cw, 0);
        int32_t n_async = 0, n_slots = 0;
        int64_t maxS = 0;
        size_t cnt_words = 0, sel_words = 0;
        for (int32_t i = 0; i < cw; ++i) {
            const int32_t gi = c0 + i;
            const mr_spans* s = spans[gi];
            bool launched = false, empty = false;
            MR_TRY(ev_partition(ctx, L, gi, slos, dstate[(size_t)i], ob.p + (size_t)i * DW, &launched, &empty, status));
            det_async[(size_t)i] = launched;
            n_async += launched;
            RpWin& w = hw[(size_t)i];
            memset(&w, 0, sizeof w);
            w.svcop = s->svcop.p;
            w.podop = s->podop.p;
            w.trace = s->trace.p;
            w.dur = s->duration.p;
            w.span = s->span.p;
            w.rank = s->rp_rank.p;
            w.pods = s->rp_pods.p;
            w.state = dstate[(size_t)i].p;
            w.n_codes = s->n_span_codes;
            w.NT = s->n_traces;
            w.NP = s->n_podops;
            for (int32_t j = 0; j < n_ops[gi]; ++j) asked[(size_t)i * K + j] = podops[(size_t)gi * K + j];
            int64_t reps = 0;
            if (!(empty || s->n_traces == 0 || s->S == 0)) reps = rp_slots(s, podops + (size_t)gi * K, n_ops[gi], w, &rep[(size_t)i * K]);
            w.direct = reps * 2 <= EV_H;
            if (reps > 0) {   // (a slot holds a replica)
                if (what == MR_LAT_SELF) {
                    MR_TRY(lat_csum_ensure(ctx, s));
                    w.csum = s->csum.p;
                }
                w.S = s->S;
                maxS = std::max<int64_t>(maxS, s->S);
            }
            cnt_at[(size_t)i] = cnt_words;
            sel_at[(size_t)i] = sel_words;
            cnt_words += (size_t)reps * 6;
            sel_words += (size_t)w.n_ops * SW;
            n_slots += w.n_ops;
        }
        DBuf<RpWin> dw;
        DBuf<int32_t> drep, dasked;
        if (n_slots > 0) {
            MR_TRY(cnt.zero(ctx, cnt_words));
            MR_TRY(sel.zero(ctx, sel_words));
            for (int32_t i = 0; i < cw; ++i) {
                hw[(size_t)i].cnt = cnt.p + cnt_at[(size_t)i];
                hw[(size_t)i].sel = sel.p + sel_at[(size_t)i];
            }
            MR_TRY(dw.upload(ctx, hw.data(), (size_t)cw));   // (hw, rep and asked live until the read-back's sync below)
            MR_TRY(drep.upload(ctx, rep.data(), rep.size()));
            MR_TRY(dasked.upload(ctx, asked.data(), asked.size()));
            // a block keeps its counters in LDS over all its tiles and adds them to the window's once: few
            // blocks per window where the chunk's windows fill the device anyway
            const int64_t rtiles = cdiv(maxS, RP_TILE);
            const int64_t rb = forced_blocks ? std::min<int64_t>(forced_blocks, rtiles)
                                             : std::min<int64_t>(rtiles, std::min<int64_t>(RP_MAX_CB, ev_block_cap(8, cw)));
            if (rb > 0)
                hipLaunchKernelGGL(k_rp_count, dim3((unsigned)rb, (unsigned)cw), dim3(RP_T), 0, st, (const RpWin*)dw.p);
            hipLaunchKernelGGL(k_rp_select, dim3((unsigned)std::min<int32_t>(K, RP_MAXOPS), (unsigned)cw), dim3(RP_T), 0, st,
                               (const RpWin*)dw.p, m);
            long long* o64 = (long long*)(ob.p + (size_t)cw * DW);
            int32_t* o32 = (int32_t*)(o64 + n64);
            const size_t n1 = (size_t)cw * KM * 2, nk = (size_t)cw * K;
            const RpOut out{o64, o64 + n1, o64 + 2 * n1, o64 + 3 * n1, o64 + 3 * n1 + nk * 6,
                            o32, o32 + (size_t)cw * KM, o32 + (size_t)cw * KM + nk, o32 + (size_t)cw * KM + 2 * nk,
                            o32 + (size_t)cw * KM + 3 * nk};
            hipLaunchKernelGGL(k_rp_finish, dim3((unsigned)K, (unsigned)cw), dim3(RP_T), 0, st, (const RpWin*)dw.p,
                               (const int32_t*)drep.p, (const int32_t*)dasked.p, K, m, out);
            MR_TRY_HIP(ctx, hipGetLastError());
        }
        if (n_slots > 0 || n_async > 0) {
            MR_TRY(mr_pin_ex(ctx, ob.p, ob_words, who));
            ev_launched_status(ctx->pin_ex, det_async, c0, status);
            if (n_slots > 0) {
                const int64_t* h64 = (const int64_t*)(ctx->pin_ex + (size_t)cw * DW);
                const int32_t* h32 = (const int32_t*)(h64 + n64);
                const size_t n1 = (size_t)cw * KM * 2, nk = (size_t)cw * K;
                memcpy(rp_cnt + (size_t)c0 * KM * 2, h64, n1 * sizeof(int64_t));
                memcpy(rp_sum + (size_t)c0 * KM * 2, h64 + n1, n1 * sizeof(int64_t));
                memcpy(rp_max + (size_t)c0 * KM * 2, h64 + 2 * n1, n1 * sizeof(int64_t));
                memcpy(rp_own + (size_t)c0 * K * 6, h64 + 3 * n1, nk * 6 * sizeof(int64_t));
                memcpy(rp_tot + (size_t)c0 * K * 6, h64 + 3 * n1 + nk * 6, nk * 6 * sizeof(int64_t));
                memcpy(rp_pod + (size_t)c0 * KM, h32, (size_t)cw * KM * sizeof(int32_t));
                memcpy(rp_n + (size_t)c0 * K, h32 + (size_t)cw * KM, nk * sizeof(int32_t));
                memcpy(rp_live + (size_t)c0 * K, h32 + (size_t)cw * KM + nk, nk * sizeof(int32_t));
                memcpy(rp_all + (size_t)c0 * K, h32 + (size_t)cw * KM + 2 * nk, nk * sizeof(int32_t));
                memcpy(rp_place + (size_t)c0 * K, h32 + (size_t)cw * KM + 3 * nk, nk * sizeof(int32_t));
                // an empty window that its launched detector found: the padding (rp_all too)
                for (int32_t gi = c0; gi < c1; ++gi)
                    if (status[gi] == MR_ERR_VALUE) std::fill(rp_all + (size_t)gi * K, rp_all + (size_t)(gi + 1) * K, (int32_t)0);
            }
        }
        c0 = c1;
    }
    return MR_OK;   // (every chunk ended in a synchronise: the pinned read-back, or a row-level detector's size read-back)
}
