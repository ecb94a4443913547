// Call evidence of a window (no reference counterpart as an entry; its counts are the multiplicities of
// preprocess_data.py:156-163's operation_operation): per asked pod-op its callers and its callees, each
// call edge with its pair count, summed child duration and largest child duration on the normal and on
// the abnormal side of the window's own detector partition.  Self-time quantiles say whether an op's own
// code is slow; this says which caller it is slow from and which dependency took the time.
//
// Everything it needs is on the device already: the spanID -> rows multimap (id_off / id_rows), the
// table's dense edge dictionary (ekey: every (parent op << 32 | child op) of T11's join over the whole
// table, ascending -- a pair's key is always in it), the detector's state byte per trace.  No layout
// order is needed, so tables of any number of pod-ops work.
//   k_ce_count   one launch for a chunk's windows, a lane per (child) row, CE_U rows in flight per
//                lane: the row's trace state first (a row outside the partition reads nothing more),
//                then its parent rows through id_off / id_rows, the parent row's trace state, and the
//                pair's dense edge id by binary search in ekey.  A window keeps whole traces (trace-level
//                times) or is the whole table, so the two states alone say that both rows lie in the
//                window.  Rows of one parent are mostly adjacent and often of one op: runs of equal
//                (edge id, side) inside a wave are reduced (mr_prim.h wave_run_reduce) and the run's
//                last lane adds calls, dsum and dmax to the block's counter table in LDS (mr_evidence.h
//                EvTable, hashed), which the block adds to the window's counters once, at its end.  A
//                spanID shared by several rows: the first parent row goes through the reduction, every
//                further one adds its own pair.  The counters are bitwise reproducible, whatever the
//                cut and whichever path a run took
//   k_ce_select  a block per (window, slice of edge ids), a thread per edge: a live edge (calls > 0 on
//                either side) whose child is asked is a caller candidate of that slot, whose parent is
//                asked a callee candidate (the asked codes, distinct, sit in LDS: at most two
//                candidates per edge).  Candidates drain into per-(slot, direction) sorted lists with
//                mr_exemplar_dev.h's ex_drain.  The list entry is (key, edge id) with
//                key = calls_abn << 32 | (0xFFFFFFFF - calls_nor): (key descending, id ascending) is
//                exactly the answer's order, because within one (slot, direction) the edge ids ascend
//                with the peer's code (ekey is sorted by parent, then child; one of the two is fixed).
//                The packed key is EXACT because the entry refuses (MR_ERR_STATE) a table whose T11
//                join has 2^32 or more pairs in all (mr_spans.n_join, counted when the table was
//                indexed): a window's count on one edge and side is at most that.  Totals (peers,
//                calls on each side) by LDS atomics and one global integer atomic per (block, list)
//   k_ce_merge   a block per (window, slot, direction) merges the blocks' lists (ex_merge_body)
//   k_ce_finish  the edge id of every answer entry into its peer code and its six counters
// One row pass per chunk of windows -- never a launch per asked op or per edge -- and one pinned
// read-back per chunk, which carries the detectors' counts too: no host synchronisation per window.  The
// window list's front end is mr_evidence.h's; a chunk's dense counters take 48 bytes per window and edge
// (MR_CE_CHUNK, read per call, forces the windows per chunk; MR_CE_BLOCKS the blocks per window of the
// count and of the select pass: tests reach every merge shape at small sizes).
#include "mr_evidence.h"
#include "mr_exemplar_dev.h"

namespace {
constexpr int CE_U = 4;                       // k_ce_count: rows in flight per lane
constexpr int CE_TILE = EX_T * CE_U;          // rows of a block's tile
constexpr int CE_L = EX_MAXOPS * 2;           // lists of a window: (slot, direction)
constexpr int CE_Q = EX_T * 2;                // most candidates of a select round
constexpr int CE_W = 6;                       // counter words per edge: [side][calls, dsum, biased dmax]
constexpr int CE_MAX_CB = 4096;               // count blocks per window (grid-stride over the tiles)

struct CeWin {
    const int32_t *podop, *trace, *id_rows;
    const int64_t *parent, *dur, *id_off;
    const uint64_t* ekey;
    const uint8_t* state;
    unsigned long long* cnt;      // [E * CE_W]
    unsigned long long* miss;     // the chunk's word of pairs whose key the edge dictionary lacks (must stay 0)
    int64_t S, n_codes, E;
    int32_t NT;
    int32_t b0, nb;               // first list block, select blocks
    int64_t per;                  // edges per select block
    int32_t n_ops;                // distinct asked codes (0: nothing is read)
    int32_t op[EX_MAXOPS];
};

// the dense id of key k in the ascending ek[0..E), or -1
__device__ __forceinline__ int64_t ce_eid(const uint64_t* __restrict__ ek, int64_t E, uint64_t k) {
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ek[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < E && ek[lo] == k ? lo : -1;
}

// (a key of the block's table: kd = edge id * 2 + side)
__global__ void __launch_bounds__(EX_T) k_ce_count(const CeWin* __restrict__ ws) {
    __shared__ EvTable tab;   // calls, dsum, biased dmax
    const CeWin& w = ws[blockIdx.y];
    const int64_t S = w.n_ops ? w.S : 0;   // (nothing asked, or an empty window: nothing is read)
    if ((int64_t)blockIdx.x * CE_TILE >= S) return;   // (block-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    tab.clear(threadIdx.x, EX_T);
    __syncthreads();
    const int64_t n_codes = w.n_codes, E = w.E;
    const uint32_t NT = (uint32_t)w.NT;
    for (int64_t base = (int64_t)blockIdx.x * CE_TILE; base < S; base += (int64_t)gridDim.x * CE_TILE) {   // (block-uniform)
        int32_t tr[CE_U];
        int st[CE_U];
#pragma unroll
        for (int k = 0; k < CE_U; ++k) {
            const int64_t c = base + k * EX_T + threadIdx.x;
            tr[k] = c < S ? w.trace[c] : -1;
        }
#pragma unroll
        for (int k = 0; k < CE_U; ++k) st[k] = (uint32_t)tr[k] < NT ? (int)w.state[tr[k]] : 0;
#pragma unroll
        for (int k = 0; k < CE_U; ++k) {
            const int64_t c = base + k * EX_T + threadIdx.x;
            int64_t kd = -1;   // (edge id, side) of the pair with the first parent row
            unsigned long long d = 0ull;
            if (st[k] == 1 || st[k] == 2) {
                const int64_t p = w.parent[c];
                if (p >= 0 && p < n_codes) {
                    const int64_t a = w.id_off[p], b = w.id_off[p + 1];
                    if (b > a) {
                        d = (unsigned long long)w.dur[c];
                        const uint64_t child = (uint64_t)(uint32_t)w.podop[c];
                        for (int64_t e = a; e < b; ++e) {
                            const int32_t r = w.id_rows[e];
                            const int32_t tp = w.trace[r];
                            if ((uint32_t)tp >= NT || (int)w.state[tp] != st[k]) continue;
                            const int64_t id = ce_eid(w.ekey, E, ((uint64_t)(uint32_t)w.podop[r] << 32) | child);
                            if (id < 0) {   // (ekey holds every pair's key: the call fails if this is ever counted)
                                atomicAdd(w.miss, 1ull);
                                continue;
                            }
                            const int64_t q = id * 2 + (st[k] - 1);
                            if (e == a) kd = q;
                            else tab.add(false, w.cnt, q, ev_run_of(true, d));
                        }
                    }
                }
            }
            EvRun run = ev_run_of(kd >= 0, d);
            const bool tail = wave_run_reduce(lane, kd, run);
            if (kd >= 0 && tail) tab.add(false, w.cnt, kd, run);
        }
    }
    __syncthreads();
    tab.flush<int64_t>(false, w.cnt, threadIdx.x, EX_T);
}

// ps / pt: [list block][KL][m]; tot: [window][KL][3] peers, abnormal, normal calls (zeroed by the caller)
__global__ void __launch_bounds__(EX_T) k_ce_select(const CeWin* __restrict__ ws, int32_t KL, int32_t m,
                                                    unsigned long long* __restrict__ ps, int32_t* __restrict__ pt,
                                                    unsigned long long* __restrict__ tot) {
    __shared__ int32_t ops[EX_MAXOPS];
    __shared__ unsigned long long ls[CE_L * EX_MAXM];   // the lists, [slot * 2 + direction][m], best first
    __shared__ int32_t lt[CE_L * EX_MAXM];
    __shared__ int32_t lc[CE_L];
    __shared__ unsigned long long qs[CE_Q];
    __shared__ int32_t qt[CE_Q];
    __shared__ unsigned char qu[CE_Q];
    __shared__ int32_t qn;
    __shared__ unsigned long long ta[CE_L], tn[CE_L];
    __shared__ uint32_t tk[CE_L];
    const CeWin& G = ws[blockIdx.y];
    const int32_t nu = G.n_ops, nl = nu * 2, lb = (int32_t)blockIdx.x;
    if (nu == 0 || lb >= G.nb) return;   // (block-uniform)
    const int tid = (int)threadIdx.x;
    if (tid < EX_MAXOPS) ops[tid] = tid < nu ? G.op[tid] : -1;
    if (tid < CE_L) {
        lc[tid] = 0;
        ta[tid] = tn[tid] = 0ull;
        tk[tid] = 0u;
    }
    __syncthreads();
    const int64_t k0 = min((int64_t)lb * G.per, G.E), k1 = min(k0 + G.per, G.E);
    for (int64_t kb = k0; kb < k1; kb += EX_T) {   // (block-uniform trip counts: barriers inside)
        if (tid == 0) qn = 0;
        __syncthreads();
        const int64_t e = kb + tid;
        if (e < k1) {
            const unsigned long long cn = G.cnt[e * CE_W], ca = G.cnt[e * CE_W + 3];
            if (cn + ca) {   // a live edge
                const uint64_t ek = G.ekey[e];
                const int32_t par = (int32_t)(ek >> 32), child = (int32_t)(uint32_t)ek;
                const unsigned long long key = (ca << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)cn);
                for (int32_t u = 0; u < nu; ++u) {
#pragma unroll
                    for (int dir = 0; dir < 2; ++dir) {
                        if (ops[u] != (dir ? par : child)) continue;
                        const int32_t l = u * 2 + dir;
                        atomicAdd(&tk[l], 1u);
                        if (ca) atomicAdd(&ta[l], ca);
                        if (cn) atomicAdd(&tn[l], cn);
                        // (the lists change only in the drain below: no race with these reads)
                        if (lc[l] == m && !ex_before(key, (int32_t)e, ls[l * m + m - 1], lt[l * m + m - 1])) continue;
                        const int32_t slot = atomicAdd(&qn, 1);
                        qs[slot] = key;
                        qt[slot] = (int32_t)e;
                        qu[slot] = (unsigned char)l;
                    }
                }
            }
        }
        __syncthreads();
        ex_drain<false>(qn, nl, m, qs, qt, qu, ls, lt, lc);
        __syncthreads();
    }
    // the block's lists, padded with (0, -1)
    const size_t ob = (size_t)(G.b0 + lb) * KL * m;
    for (int32_t i = tid; i < nl * m; i += EX_T) {
        const bool in = i % m < lc[i / m];
        ps[ob + i] = in ? ls[i] : 0ull;
        pt[ob + i] = in ? lt[i] : -1;
    }
    if (tid < nl && tk[tid]) {
        unsigned long long* t = tot + ((size_t)blockIdx.y * KL + tid) * 3;
        atomicAdd(t, (unsigned long long)tk[tid]);
        if (ta[tid]) atomicAdd(t + 1, ta[tid]);
        if (tn[tid]) atomicAdd(t + 2, tn[tid]);
    }
}

// block (window, list): the window's blocks' lists into row w * KL + list of os / ot / on
__global__ void __launch_bounds__(EX_T) k_ce_merge(const CeWin* __restrict__ ws, int32_t KL, int32_t m,
                                                   const unsigned long long* __restrict__ ps,
                                                   const int32_t* __restrict__ pt, unsigned long long* __restrict__ os,
                                                   int32_t* __restrict__ ot, int32_t* __restrict__ on) {
    const int32_t w = (int32_t)blockIdx.x / KL, l = (int32_t)blockIdx.x % KL;
    const CeWin& G = ws[w];
    if (l >= G.n_ops * 2) return;   // (uniform; on / os / ot of such a row stay the caller's zeros)
    const size_t pb = (size_t)G.b0 * KL * m, ob = (size_t)w * KL * m;
    ex_merge_body<false>(ps + pb, pt + pb, G.nb, KL, m, l, os + ob, ot + ob, on + (size_t)w * KL);
}

// entry e = (w * KL + list) * m + j: its edge id into peer [n] and val [n][6]: calls, dsum, dmax x (normal, abnormal)
__global__ void __launch_bounds__(EX_T) k_ce_finish(const CeWin* __restrict__ ws, int32_t KL, int32_t m, int64_t n,
                                                    const int32_t* __restrict__ ot, const int32_t* __restrict__ on,
                                                    int32_t* __restrict__ peer, long long* __restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * EX_T + threadIdx.x;
    if (e >= n) return;
    const int64_t row = e / m;
    const CeWin& G = ws[row / KL];
    const int32_t l = (int32_t)(row % KL);
    const bool in = l < G.n_ops * 2 && (int32_t)(e % m) < on[row];
    const int32_t id = in ? ot[e] : -1;
    long long v[6] = {0, 0, 0, 0, 0, 0};
    int32_t pc = -1;
    if (in && id >= 0 && id < G.E) {
        const uint64_t ek = G.ekey[id];
        pc = (l & 1) ? (int32_t)(uint32_t)ek : (int32_t)(ek >> 32);
        const unsigned long long* c = G.cnt + (int64_t)id * CE_W;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const unsigned long long calls = c[side * 3];
            v[side] = (long long)calls;
            v[2 + side] = (long long)c[side * 3 + 1];
            v[4 + side] = calls ? (long long)(c[side * 3 + 2] ^ EV_BIAS) : 0ll;
        }
    }
    peer[e] = pc;
#pragma unroll
    for (int k = 0; k < 6; ++k) val[e * 6 + k] = v[k];
}
}  // namespace

extern "C" int mr_windows_call_edges(mr_ctx* ctx, int32_t n_windows, const mr_spans* const* spans, const int64_t* t0,
                                     const int64_t* t1, const double* const* a3, const uint8_t* const* a3_valid,
                                     const int32_t* podops, const int32_t* n_ops, int32_t K, int32_t m, int32_t* ce_peer,
                                     int64_t* ce_calls, int64_t* ce_dsum, int64_t* ce_dmax, int32_t* ce_n,
                                     int32_t* ce_peers, int64_t* ce_tot, int32_t* status) {
    const char* who = "mr_windows_call_edges";
    const EvList L{n_windows, spans, t0, t1, a3, a3_valid, podops, n_ops, K};
    MR_TRY(ev_check_args(ctx, who, L, !n_windows || (ce_peer && ce_calls && ce_dsum && ce_dmax && ce_n && ce_peers && ce_tot && status),
                         EX_MAXOPS));
    if (m < 1 || m > EX_MAXM) return mr_fail(ctx, MR_ERR_ARG, "%s: m = %d is not in 1..%d", who, m, EX_MAXM);
    MR_TRY(ev_check_windows(ctx, who, L, false));
    for (int32_t i = 0; i < n_windows; ++i) {
        const mr_spans* s = spans[i];
        const bool whole = t0[i] == INT64_MIN && t1[i] == INT64_MAX;
        if (s->grow.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table is a trace shard of a larger table (parents may lie "
                           "on another rank)", who, i);
        if (!s->indexed || !s->ekey.p)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no per-trace index, so no edge dictionary (it is "
                           "empty, or its key bits did not fit)", who, i);
        if (!s->has_times)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no startTime/endTime columns (the window's "
                           "detector reads them, for the whole table too)", who, i);
        if (!whole && !s->uniform_times)
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has no trace-level times (a window of it cuts traces)",
                           who, i);
        if (s->n_join >= ((int64_t)1 << 32))
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table's join has %lld pairs; the select key holds counts "
                           "below 2^32", who, i, (long long)s->n_join);
        if (s->n_edge_keys >= ((int64_t)1 << 31))
            return mr_fail(ctx, MR_ERR_STATE, "%s: window %d: the table has %lld distinct call edges; a list entry holds edge "
                           "ids below 2^31", who, i, (long long)s->n_edge_keys);
    }
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (n_windows == 0) return MR_OK;
    const size_t R = (size_t)n_windows * K * 2;
    std::fill(ce_peer, ce_peer + R * m, (int32_t)-1);
    for (int64_t* p : {ce_calls, ce_dsum, ce_dmax}) std::fill(p, p + R * m * 2, (int64_t)0);
    std::fill(ce_n, ce_n + R, (int32_t)0);
    std::fill(ce_peers, ce_peers + R, (int32_t)0);
    std::fill(ce_tot, ce_tot + R * 2, (int64_t)0);
    std::fill(status, status + n_windows, (int32_t)MR_OK);
    hipStream_t st = ctx->stream;
    const int forced_chunk = knob_int("MR_CE_CHUNK"), forced_blocks = knob_int("MR_CE_BLOCKS");
    const int32_t KL = K * 2;
    const auto cnt_words = [&](int32_t i) { return (size_t)std::max<int64_t>(spans[i]->n_edge_keys, 1) * CE_W; };
    EvSlos slos;
    for (int32_t c0 = 0; c0 < n_windows;) {
        size_t words = 0;
        const int32_t c1 = ev_chunk_end(c0, n_windows, forced_chunk, 8, cnt_words, &words);
        const int32_t cw = c1 - c0;
        const size_t row = (size_t)KL * m, nm = (size_t)cw * row, CR = (size_t)cw * KL;
        std::vector<DBuf<uint8_t>> dstate((size_t)cw);
        std::vector<CeWin> hw((size_t)cw);
        std::vector<int32_t> rep((size_t)cw * K, -1);   // the slot that answers asked entry j (a duplicate: its first appearance's)
        DBuf<unsigned long long> cnt, ob;
        MR_TRY(cnt.zero(ctx, words));
        // ob, the chunk's ONE read-back: [cw * DW] the detectors' counter shards (u64), [1] pairs without an edge
        // id, [CR * 3] totals (u64), [nm] merged keys (u64), [nm * 6] values (i64), then as int32 [nm] peers, [nm]
        // merged edge ids, [CR] counts
        constexpr size_t DW = EV_DW;
        const size_t ob_words = (size_t)cw * DW + 1 + CR * 3 + nm + nm * 6 + (2 * nm + CR + 1) / 2;
        MR_TRY(ob.zero(ctx, ob_words));
        std::vector<char> det_async((size_t)cw, 0);
        int32_t n_async = 0;
        EvBlocks blocks{forced_blocks, ev_block_cap(4, cw), EX_MAXB};
        int64_t maxS = 0;
        size_t cw0 = 0;
        for (int32_t i = 0; i < cw; ++i) {
            const int32_t gi = c0 + i;
            const mr_spans* s = spans[gi];
            const int32_t NT = s->n_traces;
            // (the whole table of per-span window times goes through the row-level detector)
            bool launched = false, empty = false;
            MR_TRY(ev_partition(ctx, L, gi, slos, dstate[(size_t)i], ob.p + (size_t)i * DW, &launched, &empty, status));
            det_async[(size_t)i] = launched;
            n_async += launched;
            CeWin& w = hw[(size_t)i];
            memset(&w, 0, sizeof w);
            w.podop = s->podop.p;
            w.trace = s->trace.p;
            w.id_rows = s->id_rows.p;
            w.parent = s->parent.p;
            w.dur = s->duration.p;
            w.id_off = s->id_off.p;
            w.ekey = s->ekey.p;
            w.state = dstate[(size_t)i].p;
            w.cnt = cnt.p + cw0;
            w.miss = ob.p + (size_t)cw * DW;
            cw0 += cnt_words(gi);
            w.S = s->S;
            w.n_codes = s->n_span_codes;
            w.E = s->n_edge_keys;
            w.NT = NT;
            if (!(empty || NT == 0 || s->S == 0 || s->n_edge_keys == 0))
                ev_slots(podops + (size_t)gi * K, n_ops[gi], w.op, &w.n_ops, nullptr, &rep[(size_t)i * K]);
            blocks.add(w.E, cdiv(std::max<int64_t>(w.E, 1), EX_T), w.n_ops != 0, &w.nb, &w.per, &w.b0);
            if (w.n_ops) maxS = std::max<int64_t>(maxS, s->S);
        }
        const int64_t nblk = blocks.nblk;
        DBuf<CeWin> dw;
        DBuf<unsigned long long> ps;
        DBuf<int32_t> pt;
        if (nblk > 0) {
            MR_TRY(dw.upload(ctx, hw.data(), (size_t)cw));   // (hw lives until the read-back's sync below)
            MR_TRY(ps.alloc(ctx, (size_t)nblk * row));
            MR_TRY(pt.alloc(ctx, (size_t)nblk * row));
            unsigned long long* tot = ob.p + (size_t)cw * DW + 1;
            unsigned long long* os = tot + CR * 3;
            long long* val = (long long*)(os + nm);
            int32_t* peer = (int32_t*)(val + nm * 6);
            int32_t* ot = peer + nm;
            int32_t* on = ot + nm;
            const int64_t tiles = cdiv(maxS, CE_TILE);
            // a block keeps its counters in LDS over all its tiles and adds them to the window's once: few
            // blocks per window where the chunk's windows fill the device anyway
            const int64_t cb = forced_blocks ? std::min<int64_t>(forced_blocks, tiles)
                                             : std::min<int64_t>(tiles, std::min<int64_t>(CE_MAX_CB, ev_block_cap(8, cw)));
            hipLaunchKernelGGL(k_ce_count, dim3((unsigned)std::max<int64_t>(cb, 1), (unsigned)cw), dim3(EX_T), 0, st,
                               (const CeWin*)dw.p);
            hipLaunchKernelGGL(k_ce_select, dim3((unsigned)blocks.widest, (unsigned)cw), dim3(EX_T), 0, st, (const CeWin*)dw.p,
                               KL, m, ps.p, pt.p, tot);
            hipLaunchKernelGGL(k_ce_merge, dim3((unsigned)CR), dim3(EX_T), 0, st, (const CeWin*)dw.p, KL, m,
                               (const unsigned long long*)ps.p, (const int32_t*)pt.p, os, ot, on);
            hipLaunchKernelGGL(k_ce_finish, dim3((unsigned)cdiv((int64_t)nm, EX_T)), dim3(EX_T), 0, st, (const CeWin*)dw.p, KL,
                               m, (int64_t)nm, (const int32_t*)ot, (const int32_t*)on, peer, val);
            MR_TRY_HIP(ctx, hipGetLastError());
        }
        if (nblk > 0 || n_async > 0) {
            MR_TRY(mr_pin_ex(ctx, ob.p, ob_words, who));
            ev_launched_status(ctx->pin_ex, det_async, c0, status);
            if (ctx->pin_ex[(size_t)cw * DW])
                return mr_fail(ctx, MR_ERR_STATE, "%s: %llu call pairs have no id in their table's edge dictionary (the index "
                               "and the join disagree)", who, ctx->pin_ex[(size_t)cw * DW]);
            const unsigned long long* htot = ctx->pin_ex + (size_t)cw * DW + 1;
            const long long* hval = (const long long*)(htot + CR * 3 + nm);
            const int32_t* hpeer = (const int32_t*)(hval + nm * 6);
            const int32_t* hn = hpeer + 2 * nm;
            for (int32_t i = 0; i < (nblk > 0 ? cw : 0); ++i)
                for (int32_t j = 0; j < K; ++j) {
                    const int32_t u = rep[(size_t)i * K + j];
                    if (u < 0) continue;
                    for (int dir = 0; dir < 2; ++dir) {
                        const size_t src = (size_t)i * KL + (size_t)u * 2 + dir, dst = ((size_t)(c0 + i) * K + j) * 2 + dir;
                        memcpy(ce_peer + dst * m, hpeer + src * m, (size_t)m * sizeof(int32_t));
                        for (int32_t e = 0; e < m; ++e) {
                            const long long* v = hval + (src * m + e) * 6;
                            for (int side = 0; side < 2; ++side) {
                                ce_calls[(dst * m + e) * 2 + side] = v[side];
                                ce_dsum[(dst * m + e) * 2 + side] = v[2 + side];
                                ce_dmax[(dst * m + e) * 2 + side] = v[4 + side];
                            }
                        }
                        ce_n[dst] = hn[src];
                        ce_peers[dst] = (int32_t)htot[src * 3];
                        ce_tot[dst * 2] = (int64_t)htot[src * 3 + 2];       // side 0: normal
                        ce_tot[dst * 2 + 1] = (int64_t)htot[src * 3 + 1];   // side 1: abnormal
                    }
                }
        }
        c0 = c1;
    }
    return MR_OK;   // (every chunk ended in a synchronise: the pinned read-back, or a row-level detector's size read-back)
}
