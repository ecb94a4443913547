// Kind breakdown of a window (no reference counterpart): per asked pod-op -- and for the window as a
// whole -- the trace kinds that pass through it, each with its abnormal and normal trace count under
// the window's own detector partition.  "Every call path through the op is slow" and "one call path
// out of forty is" are different findings; this is the histogram that tells them apart.
//
// Everything it needs is on the device already: the detector's state byte per trace (mr_detect_dev)
// and the table's layout order (mr_span_index.hip lo_index), in which every exact kind class -- the
// same pod-op set, the same fp32(1 / rows) -- is a contiguous run, lo_kid the run's index, trace codes
// ascending inside a run, and a kind's op list the lo16 slice of any member.  No hash, no sort:
//   k_kb_count   one launch for a chunk's windows: a lane per layout index reads lo_kid (consecutive
//                addresses) and state[lo_tr] (the one gather), KB_U loads in flight per lane; runs of
//                equal lo_kid inside a wave are reduced by a segmented scan, and a run's last lane in
//                the wave issues the atomics -- per (window, kind) 16 bytes: the two counts and, as
//                maxima of ~layout index, the first abnormal and the first normal member.  Integer
//                adds and maxima are order-free: the counters are bitwise reproducible
//   k_kb_select  a block per (window, slice of kinds), a thread per kind: a live kind's op list (its
//                first counted member's lo16 slice, KB_U codes per round) against an LDS byte table
//                code -> asked slot; every hit, and every live kind for the slot of -1, queues
//                (key, rep trace code, slot), key = n_abn << 32 | (0xFFFFFFFF - n_nor): (key
//                descending, rep ascending) is the answer's order and exactly mr_exemplar_dev.h's,
//                so the queue drains into per-slot sorted lists in LDS as the exemplars' do
//                (ex_drain).  Totals (kinds, abnormal, normal traces per slot) by LDS atomics and one
//                global integer atomic per (block, slot, word).  43.4 KB of LDS: 4 KB table, 24.3 KB
//                lists, 13 KB queue, 1.3 KB totals
//   k_kb_merge   a block per (window, slot) merges the blocks' lists (ex_merge_body)
//   k_kb_finish  key and rep of every answer entry into the five output columns; spans and ops of
//                a kind are its rep's tlen and po_off difference (every member has the same)
// One pinned read-back per chunk.  The window list's front end is mr_evidence.h's (each window's detector
// synchronises); a chunk's dense counters take 16 bytes per window and kind (MR_KB_CHUNK, read per call,
// forces the windows per chunk; MR_KB_BLOCKS the select blocks per window: tests reach every merge shape
// at small sizes).
#include "mr_evidence.h"
#include "mr_exemplar_dev.h"

namespace {
constexpr int KB_U = 4;                       // k_kb_count: layout indices per lane; k_kb_select: codes per kind and round
constexpr int KB_PMAX = 4096;                 // pod-op codes of a table with a layout order (mr_lo_fits)
constexpr int KB_Q = EX_T * KB_U;             // most candidates of a round

struct KbWin {
    const int32_t *lo_tr, *lo_kid, *tlen;
    const int64_t *lo_off, *po_off;
    const uint16_t* lo16;
    const uint8_t* state;
    uint32_t* cnt;                // [nk * 4] n_abn, n_nor, max ~l over abnormal members, over normal members
    int32_t NT, nk;
    int32_t b0, nb, per;          // first list block, select blocks, kinds per block
    int32_t n_ops, all_slot;      // distinct asked slots; the slot of -1 (or -1: not asked)
    int32_t op[EX_MAXOPS];        // asked codes by slot (-1 at all_slot)
};

// wave_run_reduce's payload: the abnormal | normal << 16 counts of a run (<= 64 each) and the maxima of ~layout
// index over its abnormal and over its normal members
struct KbRun {
    uint32_t c, ma, mn;
    __device__ __forceinline__ KbRun up(int off) const {
        return KbRun{__shfl_up(c, off, WAVE), __shfl_up(ma, off, WAVE), __shfl_up(mn, off, WAVE)};
    }
    __device__ __forceinline__ void merge(const KbRun& lower) {
        c += lower.c;
        ma = max(ma, lower.ma);
        mn = max(mn, lower.mn);
    }
};

__global__ void __launch_bounds__(EX_T) k_kb_count(const KbWin* __restrict__ ws) {
    const KbWin& w = ws[blockIdx.y];
    const int32_t NT = w.n_ops ? w.NT : 0;   // (nothing asked, or an empty window: nothing is read)
    const int64_t base = (int64_t)blockIdx.x * (EX_T * KB_U);
    if (base >= NT) return;   // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    int32_t kid[KB_U], tr[KB_U];
    int st[KB_U];
#pragma unroll
    for (int k = 0; k < KB_U; ++k) {
        const int64_t l = base + k * EX_T + threadIdx.x;
        kid[k] = l < NT ? w.lo_kid[l] : -1;
        tr[k] = l < NT ? w.lo_tr[l] : -1;
    }
#pragma unroll
    for (int k = 0; k < KB_U; ++k) st[k] = tr[k] >= 0 ? (int)w.state[tr[k]] : 0;
#pragma unroll
    for (int k = 0; k < KB_U; ++k) {
        const uint32_t l = (uint32_t)(base + k * EX_T + threadIdx.x);
        const int32_t kd = (uint32_t)kid[k] < (uint32_t)w.nk ? kid[k] : -1;
        KbRun r{st[k] == 2 ? 1u : st[k] == 1 ? 0x10000u : 0u, st[k] == 2 ? ~l : 0u, st[k] == 1 ? ~l : 0u};   // (l < 2^31: ~l > 0)
        const bool tail = wave_run_reduce(lane, kd, r);
        if (kd >= 0 && tail && r.c) {
            uint32_t* p = w.cnt + (size_t)kd * 4;
            if (r.c & 0xFFFFu) {
                atomicAdd(p, r.c & 0xFFFFu);
                atomicMax(p + 2, r.ma);
            }
            if (r.c >> 16) {
                atomicAdd(p + 1, r.c >> 16);
                atomicMax(p + 3, r.mn);
            }
        }
    }
}

// ps / pt: [list block][KO][m]; tot: [window][KO][3] kinds, abnormal, normal traces (zeroed by the caller)
__global__ void __launch_bounds__(EX_T) k_kb_select(const KbWin* __restrict__ ws, int32_t KO, int32_t m,
                                                    unsigned long long* __restrict__ ps, int32_t* __restrict__ pt,
                                                    unsigned long long* __restrict__ tot) {
    __shared__ unsigned char tab[KB_PMAX];                   // slot of a code (0xFF: not asked)
    __shared__ unsigned long long ls[EX_MAXOPS * EX_MAXM];   // the lists, [slot][m], best first
    __shared__ int32_t lt[EX_MAXOPS * EX_MAXM];
    __shared__ int32_t lc[EX_MAXOPS];
    __shared__ unsigned long long qs[KB_Q];
    __shared__ int32_t qt[KB_Q];
    __shared__ unsigned char qu[KB_Q];
    __shared__ int32_t qn, smax;
    __shared__ unsigned long long ta[EX_MAXOPS], tn[EX_MAXOPS];
    __shared__ uint32_t tk[EX_MAXOPS];
    const KbWin& G = ws[blockIdx.y];
    const int32_t nu = G.n_ops, lb = (int32_t)blockIdx.x;
    if (nu == 0 || lb >= G.nb) return;   // (block-uniform)
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1);
    for (int i = tid; i < KB_PMAX; i += EX_T) tab[i] = 0xFF;
    if (tid < EX_MAXOPS) {
        lc[tid] = 0;
        ta[tid] = tn[tid] = 0ull;
        tk[tid] = 0u;
    }
    if (tid == 0) smax = 0;
    __syncthreads();
    if (tid < nu && (uint32_t)G.op[tid] < (uint32_t)KB_PMAX) tab[G.op[tid]] = (unsigned char)tid;
    __syncthreads();
    const int32_t all = G.all_slot;
    const int32_t k0 = (int32_t)min((int64_t)lb * G.per, (int64_t)G.nk);
    const int32_t k1 = (int32_t)min((int64_t)k0 + G.per, (int64_t)G.nk);
    for (int32_t kb = k0; kb < k1; kb += EX_T) {   // (block-uniform trip counts: barriers inside)
        const int32_t k = kb + tid;
        uint32_t na = 0, nn = 0;
        int32_t rep = -1, n = 0;
        int64_t a = 0;
        unsigned long long key = 0ull;
        if (k < k1) {
            const uint4 c = *reinterpret_cast<const uint4*>(G.cnt + (size_t)k * 4);
            na = c.x;
            nn = c.y;
            if (na + nn) {   // a live kind: its first counted member stands for it
                const uint32_t l = na ? ~c.z : ~c.w;
                rep = G.lo_tr[l];
                a = G.lo_off[l];
                n = (int32_t)(G.lo_off[l + 1] - a);
                key = ((unsigned long long)na << 32) | (unsigned long long)(0xFFFFFFFFu - nn);
            }
        }
        const bool live = rep >= 0;
        if (live) atomicMax(&smax, n);
        if (all >= 0) {   // (uniform) the whole window: every live kind
            if (tid == 0) qn = 0;
            __syncthreads();
            const int64_t wk = wave_sum_i64(live ? 1 : 0), wa = wave_sum_i64(na), wn = wave_sum_i64(nn);
            if (lane == 0 && wk) {
                atomicAdd(&tk[all], (uint32_t)wk);
                atomicAdd(&ta[all], (unsigned long long)wa);
                atomicAdd(&tn[all], (unsigned long long)wn);
            }
            // (the lists change only in the drain below: no race with these reads)
            if (live && !(lc[all] == m && !ex_before(key, rep, ls[all * m + m - 1], lt[all * m + m - 1]))) {
                const int32_t slot = atomicAdd(&qn, 1);
                qs[slot] = key;
                qt[slot] = rep;
                qu[slot] = (unsigned char)all;
            }
            __syncthreads();
            ex_drain<false>(qn, nu, m, qs, qt, qu, ls, lt, lc);
        }
        __syncthreads();
        const int32_t nmax = smax;   // the tile's longest op list
        __syncthreads();
        if (tid == 0) smax = 0;      // (for the next tile: behind every read, ahead of the tile's last barrier)
        for (int32_t r0 = 0; r0 < nmax; r0 += KB_U) {   // (uniform) KB_U codes of every kind's op list per round
            if (tid == 0) qn = 0;
            __syncthreads();
            if (r0 < n) {
                uint16_t code[KB_U];
#pragma unroll
                for (int e = 0; e < KB_U; ++e) code[e] = r0 + e < n ? G.lo16[a + r0 + e] : (uint16_t)0xFFFF;
#pragma unroll
                for (int e = 0; e < KB_U; ++e) {
                    if (code[e] >= KB_PMAX) continue;   // (past the list's end)
                    const int32_t u = tab[code[e]];
                    if (u == 0xFF) continue;
                    atomicAdd(&tk[u], 1u);
                    atomicAdd(&ta[u], (unsigned long long)na);
                    atomicAdd(&tn[u], (unsigned long long)nn);
                    if (lc[u] == m && !ex_before(key, rep, ls[u * m + m - 1], lt[u * m + m - 1])) continue;
                    const int32_t slot = atomicAdd(&qn, 1);
                    qs[slot] = key;
                    qt[slot] = rep;
                    qu[slot] = (unsigned char)u;
                }
            }
            __syncthreads();
            ex_drain<false>(qn, nu, m, qs, qt, qu, ls, lt, lc);
            __syncthreads();
        }
        __syncthreads();
    }
    // the block's lists, padded with (0, -1)
    const size_t ob = (size_t)(G.b0 + lb) * KO * m;
    for (int32_t i = tid; i < nu * m; i += EX_T) {
        const bool in = i % m < lc[i / m];
        ps[ob + i] = in ? ls[i] : 0ull;
        pt[ob + i] = in ? lt[i] : -1;
    }
    if (tid < nu && tk[tid]) {
        unsigned long long* t = tot + ((size_t)blockIdx.y * KO + tid) * 3;
        atomicAdd(t, (unsigned long long)tk[tid]);
        if (ta[tid]) atomicAdd(t + 1, ta[tid]);
        if (tn[tid]) atomicAdd(t + 2, tn[tid]);
    }
}

// block (window, slot): the window's blocks' lists into row w * KO + slot of os / ot / on
__global__ void __launch_bounds__(EX_T) k_kb_merge(const KbWin* __restrict__ ws, int32_t KO, int32_t m,
                                                   const unsigned long long* __restrict__ ps,
                                                   const int32_t* __restrict__ pt, unsigned long long* __restrict__ os,
                                                   int32_t* __restrict__ ot, int32_t* __restrict__ on) {
    const int32_t w = (int32_t)blockIdx.x / KO, u = (int32_t)blockIdx.x % KO;
    const KbWin& G = ws[w];
    if (u >= G.n_ops) return;   // (uniform; on / os / ot of such a row stay the caller's zeros)
    const size_t pb = (size_t)G.b0 * KO * m, ob = (size_t)w * KO * m;
    ex_merge_body<false>(ps + pb, pt + pb, G.nb, KO, m, u, os + ob, ot + ob, on + (size_t)w * KO);
}

// entry e = (w * KO + slot) * m + j: (key, rep) into the columns; col: [5][R * m] trace, abn, nor, spans, ops
__global__ void __launch_bounds__(EX_T) k_kb_finish(const KbWin* __restrict__ ws, int32_t KO, int32_t m, int64_t n,
                                                    const unsigned long long* __restrict__ os,
                                                    const int32_t* __restrict__ ot, const int32_t* __restrict__ on,
                                                    int32_t* __restrict__ col) {
    const int64_t e = (int64_t)blockIdx.x * EX_T + threadIdx.x;
    if (e >= n) return;
    const int64_t row = e / m;
    const KbWin& G = ws[row / KO];
    const bool in = (int32_t)(row % KO) < G.n_ops && (int32_t)(e % m) < on[row];
    const int32_t t = in ? ot[e] : -1;
    const unsigned long long key = in ? os[e] : 0ull;
    col[e] = t;
    col[n + e] = in ? (int32_t)(key >> 32) : 0;
    col[2 * n + e] = in ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : 0;
    col[3 * n + e] = in ? G.tlen[t] : 0;
    col[4 * n + e] = in ? (int32_t)(G.po_off[t + 1] - G.po_off[t]) : 0;
}
}  // namespace

extern "C" int mr_windows_kind_breakdown(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                         const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                         const int32_t* podops, const int32_t* n_ops, int32_t K, int32_t m,
                                         int32_t* kb_trace, int32_t* kb_abn, int32_t* kb_nor, int32_t* kb_spans,
                                         int32_t* kb_ops, int32_t* kb_n, int32_t* kb_kinds, int64_t* kb_tot,
                                         int32_t* status) {
    const char* who = "mr_windows_kind_breakdown";
    const EvList L{n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K};
    MR_TRY(ev_check_args(ctx, who, L, !n_windows || (kb_trace && kb_abn && kb_nor && kb_spans && kb_ops && kb_n && kb_kinds && kb_tot && status),
                         EX_MAXOPS));
    if (m < 1 || m > EX_MAXM) return mr_fail(ctx, MR_ERR_ARG, "%s: m = %d is not in 1..%d", who, m, EX_MAXM);
    MR_TRY(ev_check_windows(ctx, who, L, true));
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        if (s->grow.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table is a trace shard of a larger table (its counts would "
                           "cover this rank's traces only)", who, i);
        if (!s->indexed)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no per-trace index, so no layout order (its key "
                           "bits did not fit)", who, i);
        if (!s->uniform_times)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no trace-level times (a window of it cuts traces)",
                           who, i);
        if (!s->lo_ok || s->n_podops > KB_PMAX)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no layout order (past its pod-op, edge or count limits)",
                           who, i);
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (n_windows == 0) return MR_OK;
    const size_t R = (size_t)n_windows * K;
    std::fill(kb_trace, kb_trace + R * m, (int32_t)-1);
    for (int32_t* p : {kb_abn, kb_nor, kb_spans, kb_ops}) std::fill(p, p + R * m, (int32_t)0);
    std::fill(kb_n, kb_n + R, (int32_t)0);
    std::fill(kb_kinds, kb_kinds + R, (int32_t)0);
    std::fill(kb_tot, kb_tot + R * 2, (int64_t)0);
    std::fill(status, status + n_windows, (int32_t)MR_OK);
    hipStream_t st = ctx->stream;
    const int forced_chunk = knob_int("MR_KB_CHUNK"), forced_blocks = knob_int("MR_KB_BLOCKS");
    const auto cnt_words = [&](int32_t i) { return (size_t)std::max(spans[i]->lo_nk, 1) * 4; };   // (32-bit words)
    EvSlos slos;
    for (int32_t c0 = 0; c0 < n_windows;) {
        size_t words = 0;
        const int32_t c1 = ev_chunk_end(c0, n_windows, forced_chunk, 4, cnt_words, &words);
        const int32_t cw = c1 - c0;
        const size_t row = (size_t)K * m, nm = (size_t)cw * row, CR = (size_t)cw * K;
        std::vector<DBuf<uint8_t>> dstate((size_t)cw);
        std::vector<KbWin> hw((size_t)cw);
        std::vector<int32_t> rep(CR, -1);   // the slot that answers asked entry j (a duplicate: its first appearance's)
        DBuf<uint32_t> cnt;
        MR_TRY(cnt.zero(ctx, words));
        EvBlocks blocks{forced_blocks, ev_block_cap(4, cw), EX_MAXB};
        int64_t maxNT = 0;
        size_t cw0 = 0;
        for (int32_t i = 0; i < cw; ++i) {
            const int32_t gi = c0 + i;
            const mr_spans* s = spans[gi];
            const int32_t NT = s->n_traces;
            bool launched = false, empty = false;
            MR_TRY(ev_partition(ctx, L, gi, slos, dstate[(size_t)i], nullptr, &launched, &empty, status));
            KbWin& w = hw[(size_t)i];
            memset(&w, 0, sizeof w);
            w.lo_tr = s->lo_tr.p;
            w.lo_kid = s->lo_kid.p;
            w.tlen = s->tlen.p;
            w.lo_off = s->lo_off.p;
            w.po_off = s->po_off.p;
            w.lo16 = s->lo16.p;
            w.state = dstate[(size_t)i].p;
            w.cnt = cnt.p + cw0;
            cw0 += cnt_words(gi);
            w.NT = NT;
            w.nk = s->lo_nk;
            w.all_slot = -1;
            if (!(empty || NT == 0 || s->lo_nk == 0))
                ev_slots(podops + (size_t)gi * K, n_ops[gi], w.op, &w.n_ops, &w.all_slot, &rep[(size_t)i * K]);
            blocks.add(w.nk, cdiv(std::max(w.nk, 1), EX_T), w.n_ops != 0, &w.nb, &w.per, &w.b0);
            if (w.n_ops) maxNT = std::max<int64_t>(maxNT, NT);
        }
        const int64_t nblk = blocks.nblk;
        if (nblk > 0) {
            // ob: [CR * 3] totals (u64), [nm] merged keys (u64), then as int32 [5][nm] columns, [nm] merged reps, [CR] counts
            DBuf<KbWin> dw;
            DBuf<unsigned long long> ps, ob;
            DBuf<int32_t> pt;
            const size_t ob_words = CR * 3 + nm + (6 * nm + CR + 1) / 2;
            MR_TRY(dw.upload(ctx, hw.data(), (size_t)cw));   // (hw lives until the read-back's sync below)
            MR_TRY(ps.alloc(ctx, (size_t)nblk * row));
            MR_TRY(pt.alloc(ctx, (size_t)nblk * row));
            MR_TRY(ob.zero(ctx, ob_words));
            unsigned long long* tot = ob.p;
            unsigned long long* os = ob.p + CR * 3;
            int32_t* col = (int32_t*)(os + nm);
            int32_t* ot = col + 5 * nm;
            int32_t* on = ot + nm;
            hipLaunchKernelGGL(k_kb_count, dim3((unsigned)cdiv(maxNT, EX_T * KB_U), (unsigned)cw), dim3(EX_T), 0, st,
                               (const KbWin*)dw.p);
            hipLaunchKernelGGL(k_kb_select, dim3((unsigned)blocks.widest, (unsigned)cw), dim3(EX_T), 0, st, (const KbWin*)dw.p,
                               K, m, ps.p, pt.p, tot);
            hipLaunchKernelGGL(k_kb_merge, dim3((unsigned)CR), dim3(EX_T), 0, st, (const KbWin*)dw.p, K, m,
                               (const unsigned long long*)ps.p, (const int32_t*)pt.p, os, ot, on);
            hipLaunchKernelGGL(k_kb_finish, dim3((unsigned)cdiv((int64_t)nm, EX_T)), dim3(EX_T), 0, st, (const KbWin*)dw.p, K,
                               m, (int64_t)nm, (const unsigned long long*)os, (const int32_t*)ot, (const int32_t*)on, col);
            MR_TRY_HIP(ctx, hipGetLastError());
            MR_TRY(mr_pin_ex(ctx, ob.p, ob_words, who));
            const unsigned long long* htot = ctx->pin_ex;
            const int32_t* hcol = (const int32_t*)(ctx->pin_ex + CR * 3 + nm);
            const int32_t* hn = hcol + 6 * nm;
            int32_t* const outs[5] = {kb_trace, kb_abn, kb_nor, kb_spans, kb_ops};
            for (int32_t i = 0; i < cw; ++i)
                for (int32_t j = 0; j < K; ++j) {
                    const int32_t u = rep[(size_t)i * K + j];
                    if (u < 0) continue;
                    const size_t src = (size_t)i * K + u, dst = (size_t)(c0 + i) * K + j;
                    for (int c = 0; c < 5; ++c)
                        memcpy(outs[c] + dst * m, hcol + (size_t)c * nm + src * m, (size_t)m * sizeof(int32_t));
                    kb_n[dst] = hn[src];
                    kb_kinds[dst] = (int32_t)htot[src * 3];
                    kb_tot[dst * 2] = (int64_t)htot[src * 3 + 1];
                    kb_tot[dst * 2 + 1] = (int64_t)htot[src * 3 + 2];
                }
        }
        c0 = c1;
    }
    return MR_OK;   // (every chunk ended in a synchronise: the detector's count read-back or the pinned read-back)
}
