// Endpoint evidence of a window (no reference counterpart): a window's traces grouped by their ENTRY operation --
// the pod-op of the trace's longest root span, the user-facing endpoint -- with the count, the summed and the
// largest trace duration on the normal and on the abnormal side of the window's own detector partition; for the
// window as a whole (slot -1) and per asked pod-op, where a trace counts when it holds at least one span of the
// op, ONCE however many it holds: the first evidence that counts distinct traces per op.  It keeps one index
// per table:
//   the endpoint index (ep_index_ensure, once per table, kept on the mr_spans like rp_*), integer atomics only:
//   k_ep_max     a lane per row: atomicMax of duration ^ 2^63 into mx[trace], root rows (parent < 0) only
//   k_ep_row     a lane per row: atomicMin of the row position into row[trace], root rows that hold mx only --
//                the longest root span, ties to the first row
//   k_ep_trace   a lane per trace: ep[t] = podop[row[t]] (MR_EP_NONE without a root row), and the flag of that
//                pod-op; mr_prim's scan over the flags numbers the endpoints in code order: ep_rank[p], ep_code[],
//                their number R (kept on the host too) and ep_tr[t] = ep_rank[ep[t]], R for MR_EP_NONE: a slot
//                owns R + 1 keys
//   k_ep_count   one launch for a chunk's windows (gridDim.y).  Blocks [0, rb): a lane per entry e of the span
//                index's per-trace distinct pod-op lists (po_tr / po_op), EP_U entries in flight per lane: the
//                state of po_tr[e] first (an entry outside the partition reads nothing more), then po_op[e] and
//                its slot among the window's asked codes (at most 64, in LDS, behind a 64-bit filter of code & 63
//                in registers); only entries with a slot read ep_tr, tts and tte.  Blocks [rb, gridDim.x): the
//                slot of -1, a lane per trace.  key = ((slot * (R + 1)) + ep_tr[t]) * 2 + side; runs of equal keys
//                inside a wave are reduced (mr_prim.h wave_run_reduce) and the run's last lane adds n, the sum and
//                the maximum to the block's counter table in LDS (mr_evidence.h EvTable), direct-mapped where the
//                window's keys fit, else hashed.  The block adds its table to the window's dense counters once,
//                at its end
//   k_ep_select  a block per (window, slot) over the slot's R + 1 dense counters: mr_evidence.h ev_select_block,
//                k_rp_select's selection -- the live count, the totals, the first m live endpoints under the order
//                (abnormal count descending, normal count ascending, code ascending, MR_EP_NONE last: the key order)
//   k_ep_finish  a block per (window, asked entry): the entry's planes in their final layout from its slot's record
// One pass per chunk of windows -- never a launch per asked op or per endpoint -- and one pinned read-back per
// chunk, which carries the detectors' counts too.  The window list's front end is mr_evidence.h's (MR_EP_CHUNK,
// read per call, forces the windows per chunk; MR_EP_BLOCKS the count blocks per window and pass: tests reach
// every cut at small sizes).
#include <climits>

#include "mr_evidence.h"

namespace {
constexpr int EP_T = 256;                     // threads per block
constexpr int EP_U = 4;                       // k_ep_count: entries in flight per lane
constexpr int EP_TILE = EP_T * EP_U;          // entries (traces) of a block's tile
constexpr int EP_MAXOPS = 64;                 // asked slots per window (the evidence entries' limit)
constexpr int EP_MAXM = 32;                   // listed endpoints per asked entry
constexpr int EP_MAX_CB = 4096;               // count blocks per window and pass (grid-stride over the tiles)
constexpr int64_t EP_MAX_KEYS = (int64_t)1 << 30;   // (slot, endpoint) pairs of a window: key = pair * 2 + side is an int32

struct EpWin {
    const int32_t *po_op, *po_tr;         // the span index's per-trace distinct pod-op entries
    const int32_t *ep_tr, *code;          // the table's ep_tr [n_traces], ep_code [R]
    const long long *tts, *tte;           // [n_traces] trace-level start / end
    const uint8_t* state;
    unsigned long long* cnt;              // [n_ops * (R + 1) * 2 * 3]: slot, endpoint, side, {n, sum, biased max}
    unsigned long long* sel;              // [n_ops * (EV_SW + 7 * m)] the slots' selection records
    int64_t NE;                           // the entries of the op pass (0: no pod-op is asked)
    int32_t NT, NTp;                      // traces of the table; of the trace pass (0: -1 is not asked)
    int32_t R1;                           // R + 1: the keys of a slot
    int32_t n_ops, all_slot, direct;      // distinct asked slots; the slot of -1 (or -1); the keys fit the block's table
    int32_t op[EP_MAXOPS];                // asked codes by slot (-1 at all_slot)
};

// ---------------------------------------------------------------- the endpoint index
__global__ void __launch_bounds__(EP_T) k_ep_fill(int32_t* __restrict__ row, int32_t n) {
    const int32_t t = (int32_t)(blockIdx.x * EP_T + threadIdx.x);
    if (t < n) row[t] = INT32_MAX;
}
__global__ void __launch_bounds__(EP_T) k_ep_max(const int64_t* __restrict__ parent, const int64_t* __restrict__ dur,
                                                 const int32_t* __restrict__ trace, int64_t S, int32_t NT,
                                                 unsigned long long* __restrict__ mx) {
    const int64_t r = (int64_t)blockIdx.x * EP_T + threadIdx.x;
    if (r >= S || parent[r] >= 0) return;
    const int32_t t = trace[r];
    if ((uint32_t)t < (uint32_t)NT) atomicMax(&mx[t], (unsigned long long)dur[r] ^ EV_BIAS);
}
__global__ void __launch_bounds__(EP_T) k_ep_row(const int64_t* __restrict__ parent, const int64_t* __restrict__ dur,
                                                 const int32_t* __restrict__ trace, int64_t S, int32_t NT,
                                                 const unsigned long long* __restrict__ mx, int32_t* __restrict__ row) {
    const int64_t r = (int64_t)blockIdx.x * EP_T + threadIdx.x;
    if (r >= S || parent[r] >= 0) return;
    const int32_t t = trace[r];
    if ((uint32_t)t < (uint32_t)NT && ((unsigned long long)dur[r] ^ EV_BIAS) == mx[t]) atomicMin(&row[t], (int32_t)r);
}
__global__ void __launch_bounds__(EP_T) k_ep_trace(const int32_t* __restrict__ row, const int32_t* __restrict__ podop,
                                                   int32_t NT, int32_t NP, int32_t* __restrict__ ep,
                                                   int32_t* __restrict__ flag) {
    const int32_t t = (int32_t)(blockIdx.x * EP_T + threadIdx.x);
    if (t >= NT) return;
    const int32_t r = row[t];
    int32_t p = r != INT32_MAX ? podop[r] : MR_EP_NONE;
    if ((uint32_t)p >= (uint32_t)NP) p = MR_EP_NONE;
    ep[t] = p;
    if (p >= 0) flag[p] = 1;   // (every writer stores the same word)
}
__global__ void __launch_bounds__(EP_T) k_ep_rank(const int32_t* __restrict__ flag, const int64_t* __restrict__ off, int32_t NP,
                                                  int32_t* __restrict__ rank, int32_t* __restrict__ code) {
    const int32_t p = (int32_t)(blockIdx.x * EP_T + threadIdx.x);
    if (p >= NP) return;
    const bool is = flag[p] != 0;
    rank[p] = is ? (int32_t)off[p] : -1;
    if (is) code[off[p]] = p;   // (off[p] < off[NP] <= NP)
}
__global__ void __launch_bounds__(EP_T) k_ep_trank(const int32_t* __restrict__ ep, const int32_t* __restrict__ rank,
                                                   const int64_t* __restrict__ total, int32_t NT, int32_t* __restrict__ ep_tr) {
    const int32_t t = (int32_t)(blockIdx.x * EP_T + threadIdx.x);
    if (t >= NT) return;
    const int32_t p = ep[t];
    ep_tr[t] = p >= 0 ? rank[p] : (int32_t)*total;
}

// the table's index, built at the first call and kept
int ep_index_ensure(mr_ctx* ctx, const mr_spans* s) {
    if (s->ep_ok) return MR_OK;
    const int32_t NT = s->n_traces, NP = s->n_podops;
    const int64_t S = s->S;
    hipStream_t st = ctx->stream;
    DBuf<unsigned long long> mx;
    DBuf<int32_t> row, flag;
    DBuf<int64_t> off, tmp;
    MR_TRY(mx.zero(ctx, (size_t)std::max(NT, 1)));
    MR_TRY(row.alloc(ctx, (size_t)std::max(NT, 1)));
    MR_TRY(flag.zero(ctx, (size_t)std::max(NP, 1)));
    MR_TRY(off.zero(ctx, (size_t)NP + 1));
    MR_TRY(tmp.alloc(ctx, (size_t)std::max<int64_t>(scan_tmp_elems(std::max(NP, 1)), 1)));
    MR_TRY(s->ep.alloc(ctx, (size_t)std::max(NT, 1)));
    MR_TRY(s->ep_tr.alloc(ctx, (size_t)std::max(NT, 1)));
    MR_TRY(s->ep_rank.alloc(ctx, (size_t)std::max(NP, 1)));
    MR_TRY(s->ep_code.zero(ctx, (size_t)std::max(NP, 1)));
    int64_t R = 0;
    if (NT > 0) {
        const unsigned tb = (unsigned)cdiv(NT, EP_T);
        hipLaunchKernelGGL(k_ep_fill, dim3(tb), dim3(EP_T), 0, st, row.p, NT);
        if (S > 0) {
            const unsigned rb = (unsigned)cdiv(S, EP_T);
            hipLaunchKernelGGL(k_ep_max, dim3(rb), dim3(EP_T), 0, st, (const int64_t*)s->parent.p, (const int64_t*)s->duration.p,
                               (const int32_t*)s->trace.p, S, NT, mx.p);
            hipLaunchKernelGGL(k_ep_row, dim3(rb), dim3(EP_T), 0, st, (const int64_t*)s->parent.p, (const int64_t*)s->duration.p,
                               (const int32_t*)s->trace.p, S, NT, (const unsigned long long*)mx.p, row.p);
        }
        hipLaunchKernelGGL(k_ep_trace, dim3(tb), dim3(EP_T), 0, st, (const int32_t*)row.p, (const int32_t*)s->podop.p, NT, NP,
                           s->ep.p, flag.p);
        MR_TRY_HIP(ctx, hipGetLastError());
        if (NP > 0) {
            MR_TRY(mr_exclusive_scan_i32(ctx, flag.p, off.p, NP, tmp.p));
            hipLaunchKernelGGL(k_ep_rank, dim3((unsigned)cdiv(NP, EP_T)), dim3(EP_T), 0, st, (const int32_t*)flag.p,
                               (const int64_t*)off.p, NP, s->ep_rank.p, s->ep_code.p);
        }
        hipLaunchKernelGGL(k_ep_trank, dim3(tb), dim3(EP_T), 0, st, (const int32_t*)s->ep.p, (const int32_t*)s->ep_rank.p,
                           (const int64_t*)(off.p + NP), NT, s->ep_tr.p);
        MR_TRY_HIP(ctx, hipGetLastError());
    }
    MR_TRY(mr_read_words(ctx, off.p + NP, 1, &R));   // (syncs the stream)
    s->ep_R = (int32_t)R;
    s->ep_ok = true;
    return MR_OK;
}

// what both entries ask of a table
int ep_check_table(mr_ctx* ctx, const char* who, const mr_spans* s, int32_t i) {
    if (s->grow.p)
        return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: a trace shard of a larger table (a parent may lie on another rank, "
                       "so a root row here need not be a root)", who, i);
    return MR_OK;
}

// ---------------------------------------------------------------- the count pass
// every lane of the wave brings (kd, d), kd < 0: nothing; runs of equal keys are reduced and added once
__device__ __forceinline__ void ep_reduce(int lane, bool direct, EvTable& tab, unsigned long long* cnt, int32_t kd,
                                          unsigned long long d) {
    if (__ballot(kd >= 0) == 0ull) return;   // (wave-uniform)
    EvRun run = ev_run_of(kd >= 0, d);
    const bool tail = wave_run_reduce(lane, kd, run);
    if (kd >= 0 && tail) tab.add(direct, cnt, kd, run);
}

// blocks [0, rb) of a window: the entry pass of the op slots; [rb, gridDim.x): the trace pass of slot -1
__global__ void __launch_bounds__(EP_T) k_ep_count(const EpWin* __restrict__ ws, int32_t rb) {
    __shared__ EvTable tab;   // n, sum, biased max
    __shared__ int32_t ops[EP_MAXOPS];
    const EpWin& w = ws[blockIdx.y];
    const bool ents = (int32_t)blockIdx.x < rb;
    const int32_t bx = ents ? (int32_t)blockIdx.x : (int32_t)blockIdx.x - rb, nbx = ents ? rb : (int32_t)gridDim.x - rb;
    const int64_t N = ents ? w.NE : (int64_t)w.NTp;
    if ((int64_t)bx * EP_TILE >= N) return;   // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const bool direct = w.direct != 0;
    const int32_t n_ops = w.n_ops, R1 = w.R1;
    tab.clear(threadIdx.x, EP_T);
    if (threadIdx.x < EP_MAXOPS) ops[threadIdx.x] = (int)threadIdx.x < n_ops ? w.op[threadIdx.x] : -1;
    __syncthreads();
    const uint32_t NT = (uint32_t)w.NT;
    if (ents) {
        uint64_t filter = 0;   // bit (code & 63) of every asked code
        for (int j = 0; j < n_ops; ++j)
            if (ops[j] >= 0) filter |= 1ull << (ops[j] & 63);
        for (int64_t base = (int64_t)bx * EP_TILE; base < N; base += (int64_t)nbx * EP_TILE) {   // (block-uniform)
            int32_t tr[EP_U], po[EP_U], rk[EP_U];
            int st[EP_U], slot[EP_U];
            unsigned long long d[EP_U];
#pragma unroll
            for (int k = 0; k < EP_U; ++k) {
                const int64_t e = base + k * EP_T + threadIdx.x;
                tr[k] = e < N ? w.po_tr[e] : -1;
            }
#pragma unroll
            for (int k = 0; k < EP_U; ++k) st[k] = (uint32_t)tr[k] < NT ? (int)w.state[tr[k]] : 0;
#pragma unroll
            for (int k = 0; k < EP_U; ++k) {
                const int64_t e = base + k * EP_T + threadIdx.x;
                po[k] = st[k] == 1 || st[k] == 2 ? w.po_op[e] : -1;
            }
#pragma unroll
            for (int k = 0; k < EP_U; ++k) {
                slot[k] = -1;
                if (po[k] >= 0 && (filter >> (po[k] & 63) & 1ull))
                    for (int j = 0; j < n_ops; ++j)
                        if (ops[j] == po[k]) slot[k] = j;   // (the asked codes are distinct)
                rk[k] = -1;
                d[k] = 0ull;
                if (slot[k] >= 0) {
                    rk[k] = w.ep_tr[tr[k]];
                    d[k] = (unsigned long long)w.tte[tr[k]] - (unsigned long long)w.tts[tr[k]];
                }
            }
#pragma unroll
            for (int k = 0; k < EP_U; ++k) {
                const bool has = slot[k] >= 0 && (uint32_t)rk[k] < (uint32_t)R1;
                ep_reduce(lane, direct, tab, w.cnt, has ? (slot[k] * R1 + rk[k]) * 2 + (st[k] - 1) : -1, d[k]);
            }
        }
    } else {
        const int32_t all = w.all_slot;
        for (int64_t base = (int64_t)bx * EP_TILE; base < N; base += (int64_t)nbx * EP_TILE) {   // (block-uniform)
            int st[EP_U];
#pragma unroll
            for (int k = 0; k < EP_U; ++k) {
                const int64_t t = base + k * EP_T + threadIdx.x;
                st[k] = t < N ? (int)w.state[t] : 0;
            }
#pragma unroll
            for (int k = 0; k < EP_U; ++k) {
                const int64_t t = base + k * EP_T + threadIdx.x;
                int32_t kd = -1;
                unsigned long long d = 0ull;
                if (st[k] == 1 || st[k] == 2) {
                    const int32_t rk = w.ep_tr[t];
                    if ((uint32_t)rk < (uint32_t)R1) kd = (all * R1 + rk) * 2 + (st[k] - 1);
                    d = (unsigned long long)w.tte[t] - (unsigned long long)w.tts[t];
                }
                ep_reduce(lane, direct, tab, w.cnt, kd, d);
            }
        }
    }
    __syncthreads();
    tab.flush<int32_t>(direct, w.cnt, threadIdx.x, EP_T);
}

// ---------------------------------------------------------------- selection and the planes
// block (slot u, window): the slot's record (mr_evidence.h ev_select_block); an entry's code is the endpoint's
// pod-op code, MR_EP_NONE for the slot's last key
__global__ void __launch_bounds__(EP_T) k_ep_select(const EpWin* __restrict__ ws, int32_t m) {
    __shared__ unsigned long long tot[7];
    __shared__ EvKey wbest[EP_T / WAVE];
    const EpWin& w = ws[blockIdx.y];
    const int32_t u = (int32_t)blockIdx.x;
    if (u >= w.n_ops) return;   // (block-uniform)
    const int32_t* __restrict__ code = w.code;
    const int32_t R = w.R1 - 1;
    ev_select_block<EP_T>(w.cnt + (size_t)u * w.R1 * 6, w.R1, w.sel + (size_t)u * (EV_SW + 7 * m), m,
                          [code, R](int32_t q) { return q < R ? code[q] : (int32_t)MR_EP_NONE; }, tot, wbest);
}

// the chunk's output planes, each in the entry's final layout over the chunk's windows
struct EpOut {
    long long *cnt, *sum, *max;   // [cw * K * m * 2]
    long long* tot;               // [cw * K * 6]
    int32_t* op;                  // [cw * K * m]
    int32_t *n, *live;            // [cw * K]
};

// block (asked entry j, window): rep[window * K + j] the slot that answers the entry, or -1 (not asked, or an
// empty window: the padding)
__global__ void __launch_bounds__(EP_MAXM * 2) k_ep_finish(const EpWin* __restrict__ ws, const int32_t* __restrict__ rep,
                                                           int32_t K, int32_t m, EpOut o) {
    const EpWin& w = ws[blockIdx.y];
    const size_t x = (size_t)blockIdx.y * K + blockIdx.x;
    const int32_t u = rep[x];
    const bool on = u >= 0 && u < w.n_ops;   // (block-uniform)
    const unsigned long long* __restrict__ rec = on ? w.sel + (size_t)u * (EV_SW + 7 * m) : nullptr;
    const int32_t n = on ? (int32_t)rec[1] : 0;
    for (int32_t e = (int32_t)threadIdx.x; e < m; e += EP_MAXM * 2) {
        const bool in = e < n;
        const unsigned long long* r = in ? rec + EV_SW + (size_t)e * 7 : nullptr;
        o.op[x * m + e] = in ? (int32_t)r[0] : -1;
        for (int sd = 0; sd < 2; ++sd) {
            o.cnt[(x * m + e) * 2 + sd] = in ? (long long)r[1 + sd * 3] : 0ll;
            o.sum[(x * m + e) * 2 + sd] = in ? (long long)r[2 + sd * 3] : 0ll;
            o.max[(x * m + e) * 2 + sd] = in ? (long long)r[3 + sd * 3] : 0ll;
        }
    }
    if (threadIdx.x < 6) o.tot[x * 6 + threadIdx.x] = on ? (long long)rec[2 + threadIdx.x] : 0ll;
    if (threadIdx.x == 0) {
        o.n[x] = n;
        o.live[x] = on ? (int32_t)rec[0] : 0;
    }
}
}  // namespace

extern "C" int mr_spans_entry_ops(mr_ctx* ctx, const mr_spans* s, int32_t* ep) {
    const char* who = "mr_spans_entry_ops";
    if (!ctx || !s || s->ctx != ctx || !ep) return mr_fail(ctx, MR_ERR_ARG, "%s: bad arguments", who);
    MR_TRY(ep_check_table(ctx, who, s, 0));
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    MR_TRY(ep_index_ensure(ctx, s));
    MR_TRY(s->ep.download(ctx, ep, (size_t)s->n_traces));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MR_OK;
}

extern "C" int mr_windows_endpoints(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                    const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                    const int32_t* podops, const int32_t* n_ops, int32_t K, int32_t m, int32_t* ep_op,
                                    int64_t* ep_cnt, int64_t* ep_sum, int64_t* ep_max, int32_t* ep_n, int32_t* ep_live,
                                    int64_t* ep_tot, int32_t* status) {
    const char* who = "mr_windows_endpoints";
    const EvList L{n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K};
    MR_TRY(ev_check_args(ctx, who, L,
                         !n_windows || (ep_op && ep_cnt && ep_sum && ep_max && ep_n && ep_live && ep_tot && status),
                         EP_MAXOPS));
    if (m < 1 || m > EP_MAXM) return mr_fail(ctx, MR_ERR_ARG, "%s: m = %d is not in 1..%d", who, m, EP_MAXM);
    MR_TRY(ev_check_windows(ctx, who, L, true));
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        if (!s->indexed)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no per-trace index (it is empty, or its key bits "
                           "did not fit): its distinct pod-op lists are what the count pass reads", who, i);
        if (!s->has_times || !s->uniform_times)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no trace-level times (a trace's value is its "
                           "endTime - startTime)", who, i);
        MR_TRY(ep_check_table(ctx, who, s, i));
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (n_windows == 0) return MR_OK;
    // a window's distinct slots (the host's copy of R is what lays its counters out)
    auto slots_of = [&](int32_t i, int32_t* op, int32_t* all_slot, int32_t* rep) {
        int32_t n = 0;
        ev_slots(podops + (size_t)i * K, n_ops[i], op, &n, all_slot, rep);
        return n;
    };
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        MR_TRY(ep_index_ensure(ctx, s));
        int32_t op[EP_MAXOPS], rep[EP_MAXOPS], all = -1;
        const int64_t keys = (int64_t)slots_of(i, op, &all, rep) * ((int64_t)s->ep_R + 1);
        if (keys >= EP_MAX_KEYS)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: its asked slots hold %lld (slot, endpoint) pairs; a counter's "
                           "key holds fewer than 2^30", who, i, (long long)keys);
    }
    const size_t KM = (size_t)K * m;
    std::fill(ep_op, ep_op + (size_t)n_windows * KM, (int32_t)-1);
    for (int64_t* p : {ep_cnt, ep_sum, ep_max}) std::fill(p, p + (size_t)n_windows * KM * 2, (int64_t)0);
    for (int32_t* p : {ep_n, ep_live}) std::fill(p, p + (size_t)n_windows * K, (int32_t)0);
    std::fill(ep_tot, ep_tot + (size_t)n_windows * K * 6, (int64_t)0);
    std::fill(status, status + n_windows, (int32_t)MR_OK);
    hipStream_t st = ctx->stream;
    const int forced_chunk = knob_int("MR_EP_CHUNK"), forced_blocks = knob_int("MR_EP_BLOCKS");
    const size_t SW = (size_t)EV_SW + 7 * (size_t)m;                      // a slot's selection record
    const size_t O64 = KM * 2 * 3 + (size_t)K * 6, O32 = KM + (size_t)K * 2;   // a window's output words, int64 and int32
    EvSlos slos;
    for (int32_t c0 = 0; c0 < n_windows;) {
        size_t words = 0;
        // a window's scratch: its dense counters, its slots' records and its output planes
        const int32_t c1 = ev_chunk_end(c0, n_windows, forced_chunk, 8, [&](int32_t i) {
            int32_t op[EP_MAXOPS], rep[EP_MAXOPS], all = -1;
            const size_t ns = (size_t)slots_of(i, op, &all, rep);
            return ns * ((size_t)spans[i]->ep_R + 1) * 6 + ns * SW + O64 + (O32 + 1) / 2;
        }, &words);
        const int32_t cw = c1 - c0;
        std::vector<DBuf<uint8_t>> dstate((size_t)cw);
        std::vector<EpWin> hw((size_t)cw);
        std::vector<int32_t> rep((size_t)cw * K, -1);
        std::vector<size_t> cnt_at((size_t)cw, 0), sel_at((size_t)cw, 0);
        DBuf<unsigned long long> cnt, sel, ob;
        // ob, the chunk's ONE read-back: [cw * DW] the detectors' counter shards (u64), then the int64 planes
        // (counts, sums, maxima, totals), then the int32 planes (codes, n, live)
        constexpr size_t DW = EV_DW;
        const size_t n64 = (size_t)cw * O64, n32 = (size_t)cw * O32;
        const size_t ob_words = (size_t)cw * DW + n64 + (n32 + 1) / 2;
        MR_TRY(ob.zero(ctx, ob_words));
        std::vector<char> det_async((size_t)cw, 0);
        int32_t n_async = 0, n_slots = 0;
        int64_t maxE = 0, maxT = 0;
        size_t cnt_words = 0, sel_words = 0;
        for (int32_t i = 0; i < cw; ++i) {
            const int32_t gi = c0 + i;
            const mr_spans* s = spans[gi];
            bool launched = false, empty = false;
            MR_TRY(ev_partition(ctx, L, gi, slos, dstate[(size_t)i], ob.p + (size_t)i * DW, &launched, &empty, status));
            det_async[(size_t)i] = launched;
            n_async += launched;
            EpWin& w = hw[(size_t)i];
            memset(&w, 0, sizeof w);
            w.po_op = s->po_op.p;
            w.po_tr = s->po_tr.p;
            w.ep_tr = s->ep_tr.p;
            w.code = s->ep_code.p;
            w.tts = s->tts.p;
            w.tte = s->tte.p;
            w.state = dstate[(size_t)i].p;
            w.NT = s->n_traces;
            w.R1 = s->ep_R + 1;
            w.all_slot = -1;
            if (!empty) w.n_ops = slots_of(gi, w.op, &w.all_slot, &rep[(size_t)i * K]);
            w.direct = (int64_t)w.n_ops * w.R1 * 2 <= EV_H;
            if (w.n_ops - (w.all_slot >= 0) > 0) {   // (a pod-op is asked)
                w.NE = s->n_po;
                maxE = std::max<int64_t>(maxE, w.NE);
            }
            if (w.all_slot >= 0) {
                w.NTp = s->n_traces;
                maxT = std::max<int64_t>(maxT, w.NTp);
            }
            cnt_at[(size_t)i] = cnt_words;
            sel_at[(size_t)i] = sel_words;
            cnt_words += (size_t)w.n_ops * w.R1 * 6;
            sel_words += (size_t)w.n_ops * SW;
            n_slots += w.n_ops;
        }
        DBuf<EpWin> dw;
        DBuf<int32_t> drep;
        if (n_slots > 0) {
            MR_TRY(cnt.zero(ctx, cnt_words));
            MR_TRY(sel.zero(ctx, sel_words));
            for (int32_t i = 0; i < cw; ++i) {
                hw[(size_t)i].cnt = cnt.p + cnt_at[(size_t)i];
                hw[(size_t)i].sel = sel.p + sel_at[(size_t)i];
            }
            MR_TRY(dw.upload(ctx, hw.data(), (size_t)cw));   // (hw and rep live until the read-back's sync below)
            MR_TRY(drep.upload(ctx, rep.data(), rep.size()));
            // a block keeps its counters in LDS over all its tiles and adds them to the window's once: few
            // blocks per window where the chunk's windows fill the device anyway
            const int64_t etiles = cdiv(maxE, EP_TILE), ttiles = cdiv(maxT, EP_TILE);
            const int64_t cap = std::min<int64_t>(EP_MAX_CB, ev_block_cap(8, cw));
            const int64_t rb = forced_blocks ? std::min<int64_t>(forced_blocks, etiles) : std::min<int64_t>(etiles, cap);
            const int64_t tb = forced_blocks ? std::min<int64_t>(forced_blocks, ttiles) : std::min<int64_t>(ttiles, cap);
            if (rb + tb > 0)
                hipLaunchKernelGGL(k_ep_count, dim3((unsigned)(rb + tb), (unsigned)cw), dim3(EP_T), 0, st, (const EpWin*)dw.p,
                                   (int32_t)rb);
            hipLaunchKernelGGL(k_ep_select, dim3((unsigned)std::min<int32_t>(K, EP_MAXOPS), (unsigned)cw), dim3(EP_T), 0, st,
                               (const EpWin*)dw.p, m);
            long long* o64 = (long long*)(ob.p + (size_t)cw * DW);
            int32_t* o32 = (int32_t*)(o64 + n64);
            const size_t n1 = (size_t)cw * KM * 2, nk = (size_t)cw * K;
            const EpOut out{o64, o64 + n1, o64 + 2 * n1, o64 + 3 * n1, o32, o32 + (size_t)cw * KM, o32 + (size_t)cw * KM + nk};
            hipLaunchKernelGGL(k_ep_finish, dim3((unsigned)K, (unsigned)cw), dim3(EP_MAXM * 2), 0, st, (const EpWin*)dw.p,
                               (const int32_t*)drep.p, K, m, out);
            MR_TRY_HIP(ctx, hipGetLastError());
        }
        if (n_slots > 0 || n_async > 0) {
            MR_TRY(mr_pin_ex(ctx, ob.p, ob_words, who));
            ev_launched_status(ctx->pin_ex, det_async, c0, status);
            if (n_slots > 0) {
                const int64_t* h64 = (const int64_t*)(ctx->pin_ex + (size_t)cw * DW);
                const int32_t* h32 = (const int32_t*)(h64 + n64);
                const size_t n1 = (size_t)cw * KM * 2, nk = (size_t)cw * K;
                memcpy(ep_cnt + (size_t)c0 * KM * 2, h64, n1 * sizeof(int64_t));
                memcpy(ep_sum + (size_t)c0 * KM * 2, h64 + n1, n1 * sizeof(int64_t));
                memcpy(ep_max + (size_t)c0 * KM * 2, h64 + 2 * n1, n1 * sizeof(int64_t));
                memcpy(ep_tot + (size_t)c0 * K * 6, h64 + 3 * n1, nk * 6 * sizeof(int64_t));
                memcpy(ep_op + (size_t)c0 * KM, h32, (size_t)cw * KM * sizeof(int32_t));
                memcpy(ep_n + (size_t)c0 * K, h32 + (size_t)cw * KM, nk * sizeof(int32_t));
                memcpy(ep_live + (size_t)c0 * K, h32 + (size_t)cw * KM + nk, nk * sizeof(int32_t));
            }
        }
        c0 = c1;
    }
    return MR_OK;   // (every chunk ended in a synchronise: the pinned read-back, or a row-level detector's size read-back)
}
