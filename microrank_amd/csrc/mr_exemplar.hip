// Exemplar traces: the trace half of the personalised PageRank, and each asked op's top traces.
//
// The reference's pageRank carries two vectors (pagerank.py:116-130): the operation vector becomes
// the weights, the trace vector is request_ranking_vector (:119, :125, :127) -- how much each trace
// matters under the same personalisation.  The iteration keeps it on the device for its whole run
// and nothing fetched it: after K iterations q[K & 1] holds w_t * r'_K[t] (by position on fused
// graphs, by trace on the tile path; q32 after an fp32 ranking) and the r half of ring slot K % 3
// holds M_r(K) in MSH shards, both intact until the next set-up (the last launch cleared slot
// (K + 1) % 3, nothing runs behind the closing k_fx_b / k_iter_b but readers).
//   k_trace_rank   r_K[t] = r'_K[t] / M_r(K) by TRACE, fp64 in both precisions; r' = q / w_t.  A trace
//                  with len_t == 0 has w_t = 0, so q = 0 says nothing: its r' is (double)c_t[t] plus,
//                  where P_rs is given apart from P_sr, d * (its P_rs row's su_{K-1} sum) / M_s(K-1)
//                  -- a trace no operation_trace list names may still stand in trace_operation lists.
//                  That is k_iter_a's own expression, from what iteration K-1 read and left intact:
//                  sub[(K-1) & 1] and the s half of ring slot (K-1) % 3.  (P_rs == P_sr: the row is
//                  empty in any graph four dicts can make, r' = c_t.)  K = 0: the un-normalised
//                  1 / (N + T) of :119.
//   k_ex_select    one pass over the trace-major P_sr incidence (operation_trace: the relation
//                  `coverage` counts): per block a contiguous slice of traces, the asked ops in an
//                  LDS hash table, a top-m list per asked op in LDS; the lists go out per block.
//                  Reads: the ids once, 8 (T + 1) bytes of row starts, 8 T bytes of the vector
//   k_ex_merge     a block per asked op merges the blocks' sorted lists
//   k_win_ex_select / k_win_ex_merge   the same answer for every layout-order window graph of a window
//                  batch in one launch each (mr_windows_batch_exemplars), read from the iteration's own
//                  lane-interleaved id chunks by position: "window batches" below
// MR_EX_DISTINCT_KINDS (mr_graph_exemplars_ex, mr_windows_batch_exemplars_ex): one trace per trace kind
// (pagerank.py:54-66's exact classes), each kind by its best member under the order below, with the
// kind's class size -- compile-time variants of the same kernels (the DK template parameter); the
// plain instantiations are the code they were.
// Order: score descending, trace index ascending on equal fp64 values.  Scores are non-negative, so
// (score bits, trace index) is a total order and the answer does not depend on how the traces are cut
// into blocks (MR_EX_BLOCKS, read per call, forces the block count: tests reach the merge at tiny sizes).
#include "mr_evidence.h"       // the asked ops' slots, the list-block plan, the pinned read-back
#include "mr_exemplar_dev.h"   // the lists: order, insert, drain, merge (shared with mr_kind_breakdown.hip)
#include "mr_iter_dev.h"

constexpr int EX_HT = 256;         // slots of the asked ops' hash table (load <= 1/4)
constexpr int EX_U = 4;            // ids per thread and round of k_ex_select
constexpr int EX_Q = EX_T * EX_U;  // ids of a round: the most candidates a block queues between two drains

struct ExReq {
    int32_t n;
    int32_t op[EX_MAXOPS];   // distinct (the host answers a duplicate from its first occurrence)
};

__global__ void __launch_bounds__(EX_T) k_trace_rank(const double* __restrict__ q64, const float* __restrict__ q32,
                                                     const int32_t* __restrict__ tperm, const float* __restrict__ w_t,
                                                     const float* __restrict__ c_t,
                                                     const unsigned long long* __restrict__ mslot, int K, int32_t T,
                                                     double v0, const int64_t* __restrict__ rs_off,
                                                     const int32_t* __restrict__ rs_ops,
                                                     const double* __restrict__ su_prev, double d,
                                                     double* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    // M_r(K): the MSH r-shards of ring slot K % 3, reduced as weights_body reduces the s half;
    // M_s(K-1): the s-shards of slot (K-1) % 3
    const double Mr = wave_max(bits2d(mslot[(size_t)2 * MSH * (K % 3) + MSH + lane]));
    const double Msp = wave_max(bits2d(mslot[(size_t)2 * MSH * ((K + 2) % 3) + lane]));
    const int32_t i = (int32_t)blockIdx.x * EX_T + (int32_t)threadIdx.x;
    if (i >= T) return;
    const int32_t t = tperm ? tperm[i] : i;   // q lies by position on fused graphs
    if (K == 0) {
        out[t] = v0;
        return;
    }
    const float w = w_t[t];
    double rp;
    if (w != 0.0f) {
        rp = (q32 ? (double)q32[i] : q64[i]) / (double)w;
    } else {
        double acc = 0.0;   // (rs_off: the tile path's explicit P_rs, whose q lies by trace: i == t)
        if (rs_off)
            for (int64_t e = rs_off[t]; e < rs_off[t + 1]; ++e) acc += su_prev[rs_ops[e]];
        rp = d * (acc / Msp) + (double)c_t[t];
    }
    out[t] = rp / Mr;
}

__device__ __forceinline__ uint32_t ex_hash(int32_t op) { return ((uint32_t)op * 2654435761u) >> 24; }

// DK (MR_EX_DISTINCT_KINDS): the lists hold one trace per kind, krep[t] (the kind's first trace: the
// kinds' own exact classes) beside every candidate and entry; the lists go out with their kind ids
// (pk) and class sizes (pm = kind[trace]).  58.6 KB of LDS where the plain kernel has 46.4.
template <class ID, bool DK>
__global__ void __launch_bounds__(EX_T) k_ex_select(const int64_t* __restrict__ off, const ID* __restrict__ ids,
                                                    const double* __restrict__ trank, int32_t T, int32_t per, ExReq rq,
                                                    int32_t m, unsigned long long* __restrict__ ps,
                                                    int32_t* __restrict__ pt, const int32_t* __restrict__ krep,
                                                    const double* __restrict__ kind, int32_t* __restrict__ pk,
                                                    int32_t* __restrict__ pm) {
    __shared__ int32_t hk[EX_HT], hv[EX_HT];
    __shared__ unsigned long long ls[EX_MAXOPS * EX_MAXM];   // the lists, [op][m], best first
    __shared__ int32_t lt[EX_MAXOPS * EX_MAXM];
    __shared__ int32_t lk[DK ? EX_MAXOPS * EX_MAXM : 1];     // ... and their entries' kinds
    __shared__ int32_t lc[EX_MAXOPS];
    __shared__ unsigned long long qs[EX_Q];
    __shared__ int32_t qt[EX_Q], qu[EX_Q];
    __shared__ int32_t qk[DK ? EX_Q : 1];
    __shared__ int32_t qn;
    __shared__ int32_t so[EX_T + 1];   // a tile's row starts, relative to its first id
    __shared__ unsigned long long sr[EX_T];   // ... and its traces' scores (bits)
    const int tid = (int)threadIdx.x;
    const int32_t nu = rq.n;
    for (int i = tid; i < EX_HT; i += EX_T) hk[i] = -1;
    if (tid < EX_MAXOPS) lc[tid] = 0;
    __syncthreads();
    if (tid < nu) {
        uint32_t h = ex_hash(rq.op[tid]);
        while (atomicCAS(&hk[h], -1, rq.op[tid]) != -1) h = (h + 1) & (EX_HT - 1);
        hv[h] = tid;
    }
    __syncthreads();
    const int32_t t0 = (int32_t)min((int64_t)blockIdx.x * per, (int64_t)T);
    const int32_t t1 = (int32_t)min((int64_t)t0 + per, (int64_t)T);
    // The slice in tiles of EX_T traces (their row starts staged in LDS), a tile's ids read FLAT in
    // rounds of EX_Q: consecutive lanes, consecutive ids, EX_U independent loads per thread in
    // flight -- a walk per trace would chain one load per id and make a wave wait for its longest
    // row.  An id that is asked for finds its trace by a binary search of the row starts; a round
    // queues at most EX_Q candidates, so the queue cannot overflow.
    for (int32_t base = t0; base < t1; base += EX_T) {   // (block-uniform trip counts: barriers inside)
        const int32_t cnt = min(EX_T, t1 - base);
        const int64_t E0 = off[base];
        for (int32_t i = tid; i <= cnt; i += EX_T) so[i] = (int32_t)(off[base + i] - E0);
        if (tid < cnt) sr[tid] = d2bits(trank[base + tid]);   // (one coalesced read: no load per candidate)
        __syncthreads();
        const int32_t ne = so[cnt];
        int32_t idn[EX_U];   // the next round's ids, in flight while this round is probed and drained
#pragma unroll
        for (int k = 0; k < EX_U; ++k) {
            const int32_t x = k * EX_T + tid;
            idn[k] = x < ne ? (int32_t)ids[E0 + x] : -1;
        }
        for (int32_t r0 = 0; r0 < ne; r0 += EX_Q) {
            if (tid == 0) qn = 0;
            __syncthreads();
            int32_t id[EX_U];
#pragma unroll
            for (int k = 0; k < EX_U; ++k) {
                id[k] = idn[k];
                const int64_t x = (int64_t)r0 + EX_Q + k * EX_T + tid;
                idn[k] = x < ne ? (int32_t)ids[E0 + x] : -1;
            }
#pragma unroll
            for (int k = 0; k < EX_U; ++k) {
                if (id[k] < 0) continue;
                uint32_t h = ex_hash(id[k]);
                int32_t u = -1;
                for (int32_t key = hk[h]; key != -1; key = hk[h]) {
                    if (key == id[k]) {
                        u = hv[h];
                        break;
                    }
                    h = (h + 1) & (EX_HT - 1);
                }
                if (u < 0) continue;
                const int32_t x = r0 + k * EX_T + tid;
                int32_t lo = 0, hi = cnt;   // the row of x: the last j with so[j] <= x (empty rows share a start)
                while (hi - lo > 1) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (so[mid] <= x) lo = mid; else hi = mid;
                }
                const int32_t t = base + lo;
                const unsigned long long s = sr[lo];
                // (the lists change only in the drain below: no race with these reads)
                if (lc[u] == m && !ex_before(s, t, ls[u * m + m - 1], lt[u * m + m - 1])) continue;
                const int32_t slot = atomicAdd(&qn, 1);
                qs[slot] = s;
                qt[slot] = t;
                qu[slot] = u;
                if constexpr (DK) qk[slot] = krep[t];
            }
            __syncthreads();
            const int32_t n = qn;
            if constexpr (DK) ex_drain<true>(n, nu, m, qs, qt, qu, ls, lt, lc, qk, lk);
            else ex_drain<false>(n, nu, m, qs, qt, qu, ls, lt, lc);
            __syncthreads();
        }
        __syncthreads();   // (so[] and sr[] are rewritten by the next tile)
    }
    // the block's lists, padded with (0.0, -1)
    const size_t ob = (size_t)blockIdx.x * nu * m;
    for (int32_t i = tid; i < nu * m; i += EX_T) {
        const bool in = i % m < lc[i / m];
        ps[ob + i] = in ? ls[i] : 0ull;
        pt[ob + i] = in ? lt[i] : -1;
        if constexpr (DK) {
            pk[ob + i] = in ? lk[i] : -1;
            pm[ob + i] = in ? (int32_t)kind[lt[i]] : 0;
        }
    }
}

// out: [nu * m] scores, [nu * m] traces, [nu] counts
// (DK: the lists' kind ids pk and class sizes pm; om [nu * m] the class sizes)
template <bool DK>
__global__ void __launch_bounds__(EX_T) k_ex_merge(const unsigned long long* __restrict__ ps, const int32_t* __restrict__ pt,
                                                   int32_t nb, int32_t nu, int32_t m, unsigned long long* __restrict__ os,
                                                   int32_t* __restrict__ ot, int32_t* __restrict__ on,
                                                   const int32_t* __restrict__ pk, const int32_t* __restrict__ pm,
                                                   int32_t* __restrict__ om) {
    ex_merge_body<DK>(ps, pt, nb, nu, m, (int32_t)blockIdx.x, os, ot, on, pk, pm, om);
}

// ---------------------------------------------------------------- window batches
// The exemplars of a window batch's layout-order graphs (mr_lo_prepare_batch: no trace-major
// incidence), read from what the iteration itself walks: the lane-interleaved id chunks of the wave
// tiles (tids / coff, node ids, pads N + lane), q[K & 1] and w_tp by position, the maxima ring, and
// tcode (position -> trace code, kept for this).  One launch for every such window of the call
// (WXDev: a descriptor per window, its blocks found by a binary search as SDev / LDev); a block
// takes a contiguous range of its window's tiles, a wave a whole tile at a time: lane = position
// 64 * tile + lane, the lane's score bits computed once, one 8-byte load per lane and chunk (512 B
// per wave, coalesced: the iteration's own read), EX_U chunks in flight.  The asked ops are pod-op
// codes (the host knows no node ids): the prologue scans node_podop against them into an LDS byte
// table slot_of_node[N + 64] (0xFF: not asked; the pads land in the tail), so a probe is one LDS
// byte.  A hit queues (score bits, trace code, slot); the queue drains into the block's lists as
// k_ex_select's (ex_drain), one chunk per round -- at most EX_Q candidates.  Run-merged graphs
// (MR_TR_MERGE) hold every lane's ids, so every lane is walked, never run heads; but the merged walk
// (MR_TR_MERGE=1) writes q for a run's head only (k_tr_a: "a run's tails never read theirs"), so a
// tail takes its head's score -- the run is one kind class inside one wave tile: the same ops, w_t
// and r', which is what k_tr_a itself broadcasts (trun: the run marks, null on every other graph).
struct WXDev {
    const unsigned long long* tids;   // [chunk][lane]: four u16 node ids
    const int32_t* coff;
    const double* q64;                // slot K & 1 (one of q64 / q32)
    const float* q32;
    const float* w_tp;
    const unsigned long long* mslot;
    const int32_t *tcode, *node_podop;
    const int32_t* tkid;              // position -> the table's kind class (MR_EX_DISTINCT_KINDS), else null
    const double* kind;               // class size by position
    const uint8_t* trun;              // run marks by position (the merged walk's graphs), else null
    double v0;                        // K == 0: 1 / (N + T)
    int32_t T, N, n_wt, K, n_ops;
    int32_t b0, nb, per;              // first block, blocks, tiles per block
    int32_t op[EX_MAXOPS];            // asked pod-op codes, distinct
};
// ps / pt: [block][KO][m], padded with (0.0, -1)
// DK (MR_EX_DISTINCT_KINDS): one trace per kind.  The kind of position p is tkid[p], the table's exact
// class of its trace (a window keeps whole traces: the class restricted to the window is the window's
// kind).  Queue and lists carry the POSITION beside the score (lp; the queue in qt's place); the drain
// reads kind and trace code by position from global memory, so the kernel's LDS is the plain one's
// 38.4 KB + 8 KB of positions: 63.1 KB with the table at N = 16384, under 64 KB and two blocks per CU.
// The lists go out with their kind ids (pk) and class sizes (pm = kind[p]).
template <bool DK>
__global__ void __launch_bounds__(EX_T) k_win_ex_select(const WXDev* __restrict__ wd, int32_t nw, int32_t KO, int32_t m,
                                                        unsigned long long* __restrict__ ps, int32_t* __restrict__ pt,
                                                        int32_t* __restrict__ pk, int32_t* __restrict__ pm) {
    extern __shared__ unsigned char tab[];                   // slot_of_node[N + WAVE]
    __shared__ unsigned long long ls[EX_MAXOPS * EX_MAXM];   // the lists, [op][m], best first
    __shared__ int32_t lt[EX_MAXOPS * EX_MAXM];
    __shared__ int32_t lp[DK ? EX_MAXOPS * EX_MAXM : 1];     // ... and their entries' positions
    __shared__ int32_t lc[EX_MAXOPS];
    __shared__ unsigned long long qs[EX_T * 4];              // a round: four ids per thread
    __shared__ int32_t qt[EX_T * 4];
    __shared__ unsigned char qu[EX_T * 4];
    __shared__ int32_t qn;
    __shared__ int32_t sop[EX_MAXOPS];
    __shared__ int32_t snc[EX_T / WAVE];
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const WXDev& G = wd[block_owner<WXDev, &WXDev::b0>(wd, nw, (int32_t)blockIdx.x)];
    const int32_t N = G.N, T = G.T, K = G.K, nu = G.n_ops;
    if (tid < EX_MAXOPS) {
        lc[tid] = 0;
        sop[tid] = tid < nu ? G.op[tid] : -1;
    }
    for (int32_t o = tid; o < N + WAVE; o += EX_T) tab[o] = 0xFF;
    __syncthreads();
    for (int32_t o = tid; o < N; o += EX_T) {
        const int32_t code = G.node_podop[o];
        for (int32_t j = 0; j < nu; ++j)
            if (sop[j] == code) {
                tab[o] = (unsigned char)j;
                break;
            }
    }
    // M_r(K): the MSH r-shards of ring slot K % 3, as k_trace_rank reduces them
    const double Mr = wave_max(bits2d(G.mslot[(size_t)2 * MSH * (K % 3) + MSH + lane]));
    __syncthreads();
    const int32_t lb = (int32_t)blockIdx.x - G.b0;
    const int32_t tl0 = (int32_t)min((int64_t)lb * G.per, (int64_t)G.n_wt);
    const int32_t tl1 = (int32_t)min((int64_t)tl0 + G.per, (int64_t)G.n_wt);
    for (int32_t tb = tl0; tb < tl1; tb += EX_T / WAVE) {   // (block-uniform trip counts: barriers inside)
        const int32_t tile = tb + wv;
        const bool has = tile < tl1;
        const int32_t c0 = has ? G.coff[tile] : 0;
        const int32_t nc = has ? G.coff[tile + 1] - c0 : 0;
        const int64_t p = (int64_t)tile * WAVE + lane;
        const bool own = has && p < T;
        unsigned long long s = 0ull;
        int32_t tc = -1;
        if (own) {   // k_trace_rank's expression, by position
            tc = G.tcode[p];
            double r = G.v0;
            if (K > 0) {
                const float w = G.w_tp[p];
                const double rp = w != 0.0f ? (G.q32 ? (double)G.q32[p] : G.q64[p]) / (double)w : 0.0;
                r = rp / Mr;
            }
            s = d2bits(r);
        }
        if (G.trun) {   // (uniform) a run's tail: its head's score, the nearest head at or below this lane
            const bool hd = !own || G.trun[p] != 0;
            const unsigned long long hb = __ballot(hd) & (lane == WAVE - 1 ? ~0ull : (2ull << lane) - 1ull);
            const unsigned long long sh = __shfl(s, 63 - __builtin_clzll(hb | 1ull), WAVE);
            if (own) s = sh;
        }
        if (lane == 0) snc[wv] = nc;
        __syncthreads();
        int32_t ncmax = snc[0];
#pragma unroll
        for (int k = 1; k < EX_T / WAVE; ++k) ncmax = max(ncmax, snc[k]);
        const unsigned long long* src = G.tids + (size_t)c0 * WAVE + lane;
        unsigned long long nx[EX_U];   // the next chunks, in flight while these are probed and drained
#pragma unroll
        for (int k = 0; k < EX_U; ++k) nx[k] = k < nc ? src[(size_t)k * WAVE] : 0ull;
        for (int32_t r0 = 0; r0 < ncmax; r0 += EX_U) {
            unsigned long long cur[EX_U];
#pragma unroll
            for (int k = 0; k < EX_U; ++k) {
                cur[k] = nx[k];
                const int32_t c = r0 + EX_U + k;
                nx[k] = c < nc ? src[(size_t)c * WAVE] : 0ull;
            }
#pragma unroll
            for (int k = 0; k < EX_U; ++k) {
                if (r0 + k >= ncmax) break;   // (uniform)
                if (tid == 0) qn = 0;
                __syncthreads();
                if (own && r0 + k < nc) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int32_t id = (int32_t)((cur[k] >> (16 * e)) & 0xFFFFull);
                        if (id >= N + WAVE) continue;   // (never: ids are < N, pads N + lane, never asked)
                        const int32_t u = tab[id];
                        if (u == 0xFF) continue;
                        // (the lists change only in the drain below: no race with these reads)
                        if (lc[u] == m && !ex_before(s, tc, ls[u * m + m - 1], lt[u * m + m - 1])) continue;
                        const int32_t slot = atomicAdd(&qn, 1);
                        qs[slot] = s;
                        qt[slot] = DK ? (int32_t)p : tc;
                        qu[slot] = (unsigned char)u;
                    }
                }
                __syncthreads();
                if constexpr (DK) ex_drain<true>(qn, nu, m, qs, (const int32_t*)nullptr, qu, ls, lt, lc, qt, lp, G.tkid, G.tcode);
                else ex_drain<false>(qn, nu, m, qs, qt, qu, ls, lt, lc);
                __syncthreads();
            }
        }
        __syncthreads();   // (snc is rewritten by the next tiles)
    }
    const size_t ob = (size_t)blockIdx.x * KO * m;
    for (int32_t i = tid; i < nu * m; i += EX_T) {
        const bool in = i % m < lc[i / m];
        ps[ob + i] = in ? ls[i] : 0ull;
        pt[ob + i] = in ? lt[i] : -1;
        if constexpr (DK) {
            pk[ob + i] = in ? G.tkid[lp[i]] : -1;
            pm[ob + i] = in ? (int32_t)G.kind[lp[i]] : 0;
        }
    }
}
// block (window, op): the window's blocks' lists into row w * KO + op of os / ot / on (DK: and om)
template <bool DK>
__global__ void __launch_bounds__(EX_T) k_win_ex_merge(const WXDev* __restrict__ wd, int32_t KO, int32_t m,
                                                       const unsigned long long* __restrict__ ps,
                                                       const int32_t* __restrict__ pt, unsigned long long* __restrict__ os,
                                                       int32_t* __restrict__ ot, int32_t* __restrict__ on,
                                                       const int32_t* __restrict__ pk, const int32_t* __restrict__ pm,
                                                       int32_t* __restrict__ om) {
    const int32_t w = (int32_t)blockIdx.x / KO, u = (int32_t)blockIdx.x % KO;
    const WXDev& G = wd[w];
    if (u >= G.n_ops) return;   // (uniform; the host reads n_ops rows of a window)
    const size_t pb = (size_t)G.b0 * KO * m, ob = (size_t)w * KO * m;
    ex_merge_body<DK>(ps + pb, pt + pb, G.nb, KO, m, u, os + ob, ot + ob, on + (size_t)w * KO, DK ? pk + pb : nullptr,
                      DK ? pm + pb : nullptr, DK ? om + ob : nullptr);
}

// shard: the sharded entries' form -- this rank's traces of a graph whose last ranking was
// mr_pagerank_sharded(_converge): q holds them, the ring's r half the WHOLE graph's M_r(K)
// (rmax_take_*), sub[(K-1) & 1] and the s half are replicated, v0 counts every rank's traces
static int trace_rank_fill(mr_ctx* ctx, mr_graph* g, const char* who, bool shard) {
    if (!shard && (g->T_all != 0 || g->shard_built))
        return mr_fail(ctx, MR_ERR_STATE, "%s: a trace shard holds only its own traces (mr_graph_trace_rank_sharded / "
                       "mr_graph_exemplars_sharded answer it)", who);
    if (!g->rk_ok) return mr_fail(ctx, MR_ERR_STATE, "%s: the graph has no ranking yet", who);
    if (shard && !g->rk_sharded)
        return mr_fail(ctx, MR_ERR_STATE, "%s: the graph's last ranking was not mr_pagerank_sharded(_converge)", who);
    if (g->rk_kc)
        return mr_fail(ctx, MR_ERR_STATE, "%s: the last ranking was MR_PR_KIND_COMPRESS (its trace vector is the kinds')", who);
    if (g->lo || (g->fused && !g->tperm.p && g->T > 0))
        return mr_fail(ctx, MR_ERR_STATE, "%s: a layout-order window graph has no trace-major incidence", who);
    if (g->trank_ok) return MR_OK;
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t T = g->T, K = g->rk_iters;
    MR_TRY(g->trank.alloc(ctx, (size_t)T));
    const double* q64 = g->rk_fp32 ? nullptr : g->q64[K & 1].p;
    const float* q32 = g->rk_fp32 ? g->q32[K & 1].p : nullptr;
    if (K > 0 && T > 0 && !(g->rk_fp32 ? (const void*)q32 : (const void*)q64))
        return mr_fail(ctx, MR_ERR_STATE, "%s: the ranking's trace vector is gone", who);
    // the P_rs rows of traces with w_t = 0: only where P_rs is given apart from P_sr (never fused)
    const bool rs_rows = !g->rs_is_sr && !g->fused && K > 0 && g->sub[(K + 1) & 1].p;
    const int64_t T_all = shard && g->T_all > 0 ? g->T_all : (int64_t)T;
    if (T > 0)   // (a shard may hold no trace)
        hipLaunchKernelGGL(k_trace_rank, dim3(cdiv(T, EX_T)), dim3(EX_T), 0, ctx->stream, q64, q32,
                           g->fused ? (const int32_t*)g->tperm.p : (const int32_t*)nullptr, g->w_t.p, g->c_t.p, g->mslot.p, K, T,
                           1.0 / (double)((int64_t)g->N + T_all), rs_rows ? (const int64_t*)g->rs_off.p : (const int64_t*)nullptr,
                           (const int32_t*)g->rs_ops.p, (const double*)g->sub[(K + 1) & 1].p, g->rk_d, g->trank.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    g->trank_ok = true;
    return MR_OK;
}
int mr_trace_rank_ensure(mr_ctx* ctx, mr_graph* g, const char* who) { return trace_rank_fill(ctx, g, who, false); }

// request_ranking_vector after the last ranking's iterations (pagerank.py:119-127), in the graph's trace order
extern "C" int mr_graph_trace_rank(mr_graph* g, double* r) {
    if (!g) return MR_ERR_ARG;
    mr_ctx* ctx = g->ctx;
    if (!r) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_trace_rank: null argument");
    MR_TRY(mr_trace_rank_ensure(ctx, g, "mr_graph_trace_rank"));
    MR_TRY(g->trank.download(ctx, r, (size_t)g->T));
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MR_OK;
}

// distinct ops for the kernels; request i is answered from slot[i]
static void ex_request(const int32_t* ops, int32_t n_ops, ExReq& rq, int32_t* slot) {
    memset(&rq, 0, sizeof rq);
    ev_slots(ops, n_ops, rq.op, &rq.n, nullptr, slot);
}
// A graph's own lists for a request: k_ex_select over its traces, k_ex_merge over the blocks, into ob --
// [nu * m] score bits, then as int32 [nu * m] traces, [nu] counts and (dk) [nu * m] class sizes.  The
// scratch lives here until the caller's sync.  A graph without traces (an empty shard): zero counts.
struct ExLists {
    DBuf<unsigned long long> ps, ob;
    DBuf<int32_t> pt, pk, pm;
    size_t nm = 0, ob_words = 0;
};
static int ex_local_lists(mr_ctx* ctx, mr_graph* g, const ExReq& rq, int32_t m, bool dk, ExLists& L) {
    const int32_t T = g->T, nu = rq.n;
    const size_t nm = L.nm = (size_t)nu * m;
    L.ob_words = nm + (nm + (size_t)nu + (dk ? nm : 0) + 1) / 2;
    hipStream_t st = ctx->stream;
    // the P_sr rows, trace-major: operation_trace as uploaded, else the one incidence of P_rs == P_sr
    // (T == 0, an empty shard: one block that reads nothing and writes empty lists)
    const int64_t* off = g->rs_is_sr ? g->rs_off.p : g->srt_off.p;
    if (!off && T > 0) return mr_fail(ctx, MR_ERR_STATE, "mr_graph_exemplars: the graph has no trace-major incidence");
    EvBlocks blocks{knob_int("MR_EX_BLOCKS"), ev_block_cap(2, 1), EX_MAXB};
    int32_t nb = 0, per = 0, b0 = 0;
    blocks.add(T, cdiv(std::max(T, 1), EX_T), true, &nb, &per, &b0);
    MR_TRY(L.ps.alloc(ctx, (size_t)nb * nm));
    MR_TRY(L.pt.alloc(ctx, (size_t)nb * nm));
    if (dk) {
        if (!g->kind.p || !g->krep.p) return mr_fail(ctx, MR_ERR_STATE, "mr_graph_exemplars_ex: the graph's kinds are gone");
        MR_TRY(L.pk.alloc(ctx, (size_t)nb * nm));
        MR_TRY(L.pm.alloc(ctx, (size_t)nb * nm));
    }
    MR_TRY(L.ob.alloc(ctx, L.ob_words));
    const int32_t* krep = dk ? (const int32_t*)g->krep.p : (const int32_t*)nullptr;
    const double* kind = dk ? (const double*)g->kind.p : (const double*)nullptr;
    auto sel16 = dk ? k_ex_select<uint16_t, true> : k_ex_select<uint16_t, false>;
    auto sel32 = dk ? k_ex_select<int32_t, true> : k_ex_select<int32_t, false>;
    if (g->rs_is_sr && g->rs16.p)
        hipLaunchKernelGGL(sel16, dim3((unsigned)nb), dim3(EX_T), 0, st, off, (const uint16_t*)g->rs16.p,
                           (const double*)g->trank.p, T, per, rq, m, L.ps.p, L.pt.p, krep, kind, L.pk.p, L.pm.p);
    else
        hipLaunchKernelGGL(sel32, dim3((unsigned)nb), dim3(EX_T), 0, st, off,
                           g->rs_is_sr ? (const int32_t*)g->rs_ops.p : (const int32_t*)g->srt_ops.p,
                           (const double*)g->trank.p, T, per, rq, m, L.ps.p, L.pt.p, krep, kind, L.pk.p, L.pm.p);
    int32_t* ot = (int32_t*)(L.ob.p + nm);
    hipLaunchKernelGGL(dk ? k_ex_merge<true> : k_ex_merge<false>, dim3((unsigned)nu), dim3(EX_T), 0, st,
                       (const unsigned long long*)L.ps.p, (const int32_t*)L.pt.p, (int32_t)nb, nu, m, L.ob.p, ot, ot + nm,
                       (const int32_t*)L.pk.p, (const int32_t*)L.pm.p, ot + nm + nu);
    MR_TRY_HIP(ctx, hipGetLastError());
    return MR_OK;
}

// include/microrank_hip.h.  flags == 0: the plain kernels, launches and read-back.  MR_EX_DISTINCT_KINDS:
// the kinds' representatives (g->krep, built at the first such call on the graph: mr_kind_reps_ensure)
// beside the trace vector, the DK instantiations, and the class sizes behind the counts in the same
// read-back.
extern "C" int mr_graph_exemplars_ex(mr_graph* g, const int32_t* ops, int32_t n_ops, int32_t m, uint32_t flags,
                                     int32_t* out_trace, double* out_score, int32_t* out_n, int32_t* out_mult) {
    if (!g) return MR_ERR_ARG;
    mr_ctx* ctx = g->ctx;
    if (!ops || !out_trace || !out_score || !out_n) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_exemplars: null argument");
    if (flags & ~(uint32_t)MR_EX_DISTINCT_KINDS) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_exemplars_ex: unknown flag bits 0x%x", flags);
    const bool dk = (flags & MR_EX_DISTINCT_KINDS) != 0;
    if (!dk && out_mult) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_exemplars_ex: out_mult without MR_EX_DISTINCT_KINDS");
    if (n_ops < 1 || n_ops > EX_MAXOPS) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_exemplars: n_ops outside 1..%d", EX_MAXOPS);
    if (m < 1 || m > EX_MAXM) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_exemplars: m outside 1..%d", EX_MAXM);
    for (int32_t i = 0; i < n_ops; ++i)
        if (ops[i] < 0 || ops[i] >= g->N) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_exemplars: op %d outside [0, %d)", ops[i], g->N);
    MR_TRY(mr_trace_rank_ensure(ctx, g, "mr_graph_exemplars"));
    if (dk) MR_TRY(mr_kind_reps_ensure(ctx, g));
    ExReq rq;
    int32_t slot[EX_MAXOPS];
    ex_request(ops, n_ops, rq, slot);
    const int32_t nu = rq.n;
    ExLists L;
    MR_TRY(ex_local_lists(ctx, g, rq, m, dk, L));
    const size_t nm = L.nm, ob_words = L.ob_words;
    unsigned char* h = nullptr;   // <= 64 * 32 * 16 + 64 * 4 + 8 bytes: one pinned read-back
    MR_TRY(mr_read_bytes(ctx, L.ob.p, ob_words * sizeof(unsigned long long), &h));
    const double* hs = (const double*)h;
    const int32_t* hts = (const int32_t*)(h + nm * sizeof(double));
    const int32_t* hn = hts + nm;
    const int32_t* hm = hn + nu;
    for (int32_t i = 0; i < n_ops; ++i) {
        const size_t u = (size_t)slot[i];
        memcpy(out_score + (size_t)i * m, hs + u * m, (size_t)m * sizeof(double));
        memcpy(out_trace + (size_t)i * m, hts + u * m, (size_t)m * sizeof(int32_t));
        out_n[i] = hn[u];
        if (out_mult) memcpy(out_mult + (size_t)i * m, hm + u * m, (size_t)m * sizeof(int32_t));
    }
    return MR_OK;
}
extern "C" int mr_graph_exemplars(mr_graph* g, const int32_t* ops, int32_t n_ops, int32_t m, int32_t* out_trace,
                                  double* out_score, int32_t* out_n) {
    return mr_graph_exemplars_ex(g, ops, n_ops, m, 0u, out_trace, out_score, out_n, nullptr);
}

// ---------------------------------------------------------------- trace shards
// The same two answers after mr_pagerank_sharded(_converge), where each rank holds only its own traces.
// The trace vector needs no exchange: q[K & 1] is this rank's, the ring's r half already holds the
// WHOLE graph's M_r(K) (every rank's r' maximum rides the per-iteration all-reduce).  The exemplars
// are each rank's own lists (k_ex_select + k_ex_merge, as on a whole graph), then
//   k_ex_shard_pack    every list entry as a (score bits, global trace id) record into a send buffer of
//                      FIXED size -- the maxima EX_MAXOPS x EX_MAXM records, EX_MAXOPS counts and a
//                      header (n_ops, m, the ranking's iterations and precision, a hash of the ops) --
//                      so that a rank asking something else cannot desynchronise the all-gather
//   one mr_coll_allgather
//   k_ex_shard_merge   a block per op, a thread per rank: m rounds of "best head" over the ranks'
//                      sorted lists, score bits descending, global id ascending; block 0 compares the
//                      headers.  A trace lies on one rank, so the winner's id names its list.
constexpr int XS_HDR = 8;                                                       // header words
constexpr int XS_WORDS = XS_HDR + EX_MAXOPS + 2 * EX_MAXOPS * EX_MAXM;          // u64 words a rank sends
struct XsHdr {
    unsigned long long w[XS_HDR];
};

__global__ void __launch_bounds__(EX_T) k_ex_shard_pack(const unsigned long long* __restrict__ os,
                                                        const int32_t* __restrict__ ot, const int32_t* __restrict__ on,
                                                        int32_t nu, int32_t m, const int32_t* __restrict__ trace_code,
                                                        long long base, XsHdr hdr, unsigned long long* __restrict__ send) {
    const int32_t i = (int32_t)blockIdx.x * EX_T + (int32_t)threadIdx.x;   // entry (u, j) of the maxima
    if (i >= EX_MAXOPS * EX_MAXM) return;
    if (i < XS_HDR) send[i] = hdr.w[i];
    const int32_t u = i / EX_MAXM, j = i % EX_MAXM;
    const int32_t c = u < nu ? min(on[u], m) : 0;
    if (j == 0) send[XS_HDR + u] = (unsigned long long)c;
    ulonglong2 rec = make_ulonglong2(0ull, ~0ull);   // absent: (0.0, -1)
    if (j < c) {
        const int32_t t = ot[(size_t)u * m + j];
        rec.x = os[(size_t)u * m + j];
        rec.y = (unsigned long long)(trace_code ? (long long)trace_code[t] : base + t);
    }
    *reinterpret_cast<ulonglong2*>(send + XS_HDR + EX_MAXOPS + 2 * (size_t)i) = rec;   // (16-byte aligned: an even word)
}

__device__ __forceinline__ bool xs_before(unsigned long long s, long long g, unsigned long long s2, long long g2) {
    return s > s2 || (s == s2 && g < g2);
}
// recv: R ranks' send buffers; os / og [nu * m], on [nu], bad [1] (headers differ)
__global__ void __launch_bounds__(EX_T) k_ex_shard_merge(const unsigned long long* __restrict__ recv, int32_t R, int32_t m,
                                                         unsigned long long* __restrict__ os, long long* __restrict__ og,
                                                         int32_t* __restrict__ on, int32_t* __restrict__ bad) {
    __shared__ unsigned long long rs[EX_T / WAVE];
    __shared__ long long rg[EX_T / WAVE];
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const int32_t u = (int32_t)blockIdx.x;
    const bool has = tid < R;   // (R <= EX_T: the host checks)
    const unsigned long long* mine = recv + (size_t)(has ? tid : 0) * XS_WORDS;
    if (u == 0) {   // every rank asked the same of the same ranking
        int diff = 0;
        if (has)
            for (int k = 0; k < XS_HDR; ++k) diff |= mine[k] != recv[k];
        diff = __syncthreads_or(diff);
        if (tid == 0) *bad = diff;
    }
    // this thread's list: rank tid's entries of op u, sorted (the layout does not depend on m)
    const ulonglong2* list = reinterpret_cast<const ulonglong2*>(mine + XS_HDR + EX_MAXOPS) + (size_t)u * EX_MAXM;
    const int32_t c = has ? (int32_t)min(mine[XS_HDR + u], (unsigned long long)EX_MAXM) : 0;
    int32_t hp = 0;
    unsigned long long hs = 0ull;
    long long hg = -1;   // (-1: the list is used up)
    if (hp < c) {
        const ulonglong2 e = list[0];
        hs = e.x;
        hg = (long long)e.y;
    }
    int32_t cnt = 0;
    for (int32_t j = 0; j < m; ++j) {
        unsigned long long bs = hs;
        long long bg = hg;
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) {
            const unsigned long long s2 = __shfl_xor(bs, d, WAVE);
            const long long g2 = __shfl_xor(bg, d, WAVE);
            if (g2 >= 0 && (bg < 0 || xs_before(s2, g2, bs, bg))) {
                bs = s2;
                bg = g2;
            }
        }
        __syncthreads();   // (the previous round's reads of rs / rg)
        if (lane == 0) {
            rs[wv] = bs;
            rg[wv] = bg;
        }
        __syncthreads();
        bs = rs[0];
        bg = rg[0];
        for (int w = 1; w < EX_T / WAVE; ++w)
            if (rg[w] >= 0 && (bg < 0 || xs_before(rs[w], rg[w], bs, bg))) {
                bs = rs[w];
                bg = rg[w];
            }
        if (bg < 0) break;   // (uniform) every list is used up
        if (tid == 0) {
            os[(size_t)u * m + j] = bs;
            og[(size_t)u * m + j] = bg;
        }
        ++cnt;
        if (hg == bg) {   // this rank's head won: its next entry
            ++hp;
            hs = 0ull;
            hg = -1;
            if (hp < c) {
                const ulonglong2 e = list[hp];
                hs = e.x;
                hg = (long long)e.y;
            }
        }
    }
    for (int32_t j = cnt + tid; j < m; j += EX_T) {
        os[(size_t)u * m + j] = 0ull;
        og[(size_t)u * m + j] = -1;
    }
    if (tid == 0) on[u] = cnt;
}

// r of this rank's traces after the last sharded ranking, normalised by the whole graph's M_r(K), and
// the traces' global ids (the codes of a span-built shard, else t_base + t: shard_exchange)
extern "C" int mr_graph_trace_rank_sharded(mr_graph* g, double* r, int64_t* gid) {
    if (!g) return MR_ERR_ARG;
    mr_ctx* ctx = g->ctx;
    if (!r) return mr_fail(ctx, MR_ERR_ARG, "mr_graph_trace_rank_sharded: null argument");
    MR_TRY(trace_rank_fill(ctx, g, "mr_graph_trace_rank_sharded", true));
    const size_t T = (size_t)g->T;
    std::vector<int32_t> code;
    MR_TRY(g->trank.download(ctx, r, T));
    if (gid && g->shard_built && T) {
        if (!g->trace_code.p) return mr_fail(ctx, MR_ERR_STATE, "mr_graph_trace_rank_sharded: the graph's trace codes are gone");
        code.resize(T);
        MR_TRY(g->trace_code.download(ctx, code.data(), T));
    }
    MR_TRY_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (gid)
        for (size_t t = 0; t < T; ++t) gid[t] = g->shard_built ? (int64_t)code[t] : g->t_base + (int64_t)t;
    return MR_OK;
}

extern "C" int mr_graph_exemplars_sharded(mr_graph* g, const int32_t* ops, int32_t n_ops, int32_t m, int64_t* out_trace,
                                          double* out_score, int32_t* out_n) {
    if (!g) return MR_ERR_ARG;
    mr_ctx* ctx = g->ctx;
    const char* who = "mr_graph_exemplars_sharded";
    if (!ops || !out_trace || !out_score || !out_n) return mr_fail(ctx, MR_ERR_ARG, "%s: null argument", who);
    if (n_ops < 1 || n_ops > EX_MAXOPS) return mr_fail(ctx, MR_ERR_ARG, "%s: n_ops outside 1..%d", who, EX_MAXOPS);
    if (m < 1 || m > EX_MAXM) return mr_fail(ctx, MR_ERR_ARG, "%s: m outside 1..%d", who, EX_MAXM);
    for (int32_t i = 0; i < n_ops; ++i)
        if (ops[i] < 0 || ops[i] >= g->N) return mr_fail(ctx, MR_ERR_ARG, "%s: op %d outside [0, %d)", who, ops[i], g->N);
    const int R = ctx->nranks;
    if (R > EX_T) return mr_fail(ctx, MR_ERR_ARG, "%s: more than %d ranks", who, EX_T);
    MR_TRY(trace_rank_fill(ctx, g, who, true));
    if (g->shard_built && g->T > 0 && !g->trace_code.p) return mr_fail(ctx, MR_ERR_STATE, "%s: the graph's trace codes are gone", who);
    ExReq rq;
    int32_t slot[EX_MAXOPS];
    ex_request(ops, n_ops, rq, slot);
    const int32_t nu = rq.n;
    ExLists L;
    MR_TRY(ex_local_lists(ctx, g, rq, m, false, L));
    XsHdr hdr;
    memset(&hdr, 0, sizeof hdr);
    unsigned long long hash = 1469598103934665603ull;   // FNV-1a over the request's ops, in order
    for (int32_t i = 0; i < n_ops; ++i) hash = (hash ^ (uint32_t)ops[i]) * 1099511628211ull;
    hdr.w[0] = (unsigned long long)n_ops;
    hdr.w[1] = (unsigned long long)m;
    hdr.w[2] = (unsigned long long)g->rk_iters;
    hdr.w[3] = g->rk_fp32 ? 1ull : 0ull;
    hdr.w[4] = hash;
    hipStream_t st = ctx->stream;
    const size_t nm = L.nm;
    // out: [nu * m] score bits, [nu * m] global ids, then as int32 [nu] counts and the header word
    const size_t out_words = 2 * nm + ((size_t)nu + 1 + 1) / 2;
    DBuf<unsigned long long> send, recv, out;
    MR_TRY(send.alloc(ctx, XS_WORDS));
    MR_TRY(recv.alloc(ctx, (size_t)XS_WORDS * R));
    MR_TRY(out.alloc(ctx, out_words));
    const int32_t* lt = (const int32_t*)(L.ob.p + nm);
    hipLaunchKernelGGL(k_ex_shard_pack, dim3(cdiv(EX_MAXOPS * EX_MAXM, EX_T)), dim3(EX_T), 0, st,
                       (const unsigned long long*)L.ob.p, lt, lt + nm, nu, m,
                       g->shard_built ? (const int32_t*)g->trace_code.p : (const int32_t*)nullptr, (long long)g->t_base, hdr,
                       send.p);
    MR_TRY_HIP(ctx, hipGetLastError());
    MR_TRY(mr_coll_allgather(ctx, send.p, recv.p, XS_WORDS, MR_DT_U64));
    int32_t* oi = (int32_t*)(out.p + 2 * nm);
    hipLaunchKernelGGL(k_ex_shard_merge, dim3((unsigned)nu), dim3(EX_T), 0, st, (const unsigned long long*)recv.p, (int32_t)R, m,
                       out.p, (long long*)(out.p + nm), oi, oi + nu);
    MR_TRY_HIP(ctx, hipGetLastError());
    unsigned char* h = nullptr;   // <= 64 * 32 * 16 + 65 * 4 + 4 bytes: one pinned read-back
    MR_TRY(mr_read_bytes(ctx, out.p, out_words * sizeof(unsigned long long), &h));
    const double* hs = (const double*)h;
    const int64_t* hg = (const int64_t*)(h + nm * sizeof(double));
    const int32_t* hn = (const int32_t*)(h + 2 * nm * sizeof(double));
    if (hn[nu])
        return mr_fail(ctx, MR_ERR_ARG, "%s: the ranks' requests differ (ops, m) or follow different rankings", who);
    for (int32_t i = 0; i < n_ops; ++i) {
        const size_t u = (size_t)slot[i];
        memcpy(out_score + (size_t)i * m, hs + u * m, (size_t)m * sizeof(double));
        memcpy(out_trace + (size_t)i * m, hg + u * m, (size_t)m * sizeof(int64_t));
        out_n[i] = hn[u];
    }
    return MR_OK;
}

// The window batch's exemplar rows (mr_internal.h): every layout-order window of the call in one
// k_win_ex_select + one k_win_ex_merge + one pinned read-back; a window with a trace-major
// incidence (no layout order, per-span times, wide) through mr_graph_exemplars on the record of
// its ranking, trace index -> trace_code.  Blocks per window: a block per 16 wave tiles, at most
// its share of four blocks per CU (MR_EX_BLOCKS, read per call, forces the count).
int mr_win_exemplars(mr_ctx* ctx, const MrWinEx* ws, int n, int32_t m, uint32_t flags) {
    if (n <= 0) return MR_OK;
    if (m < 1 || m > EX_MAXM) return mr_fail(ctx, MR_ERR_ARG, "mr_win_exemplars: m outside 1..%d", EX_MAXM);
    const bool dk = (flags & MR_EX_DISTINCT_KINDS) != 0;
    MR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<int> lo;
    for (int k = 0; k < n; ++k) {
        const MrWinEx& w = ws[k];
        if (!w.g || w.n_ops < 0 || w.n_ops > EX_MAXOPS) return mr_fail(ctx, MR_ERR_ARG, "mr_win_exemplars: bad window");
        for (int32_t j = 0; j < w.n_ops; ++j) w.cnt[j] = 0;
        for (size_t j = 0; j < (size_t)w.n_ops * m; ++j) {
            w.trace[j] = -1;
            w.score[j] = 0.0;
            if (w.mult) w.mult[j] = 0;
        }
        if (w.n_ops && w.g->lo) lo.push_back(k);
    }
    if (!lo.empty()) {
        const int nw = (int)lo.size();
        EvBlocks blocks{knob_int("MR_EX_BLOCKS"), ev_block_cap(4, nw), EX_MAXB};
        std::vector<WXDev> hd((size_t)nw);
        int32_t KO = 1, maxN = 0;
        for (int i = 0; i < nw; ++i) {
            const MrWinEx& w = ws[lo[(size_t)i]];
            const mr_graph* g = w.g;
            WXDev& v = hd[(size_t)i];
            memset(&v, 0, sizeof v);
            const void* q = w.fp32 ? (const void*)g->q32[w.K & 1].p : (const void*)g->q64[w.K & 1].p;
            if (!g->tcode.p || !g->tids.p || !g->coff.p || !g->w_tp.p || !g->mslot.p || !g->node_podop.p || !q || w.K < 0 ||
                g->N <= 0 || g->T <= 0 || g->N + WAVE > 65536 || g->n_wt != cdiv(g->T, WAVE) ||
                (dk && (!g->tkid.p || !g->kind.p)))
                return mr_fail(ctx, MR_ERR_STATE, "mr_win_exemplars: a layout-order window graph without the ranking's state");
            v.tids = (const unsigned long long*)g->tids.p;
            v.coff = g->coff.p;
            v.q64 = w.fp32 ? nullptr : g->q64[w.K & 1].p;
            v.q32 = w.fp32 ? g->q32[w.K & 1].p : nullptr;
            v.w_tp = g->w_tp.p;
            v.mslot = g->mslot.p;
            v.tcode = g->tcode.p;
            v.node_podop = g->node_podop.p;
            v.tkid = dk ? g->tkid.p : nullptr;
            v.kind = g->kind.p;
            v.trun = g->lo_merged == 1 ? g->trun.p : nullptr;   // (as the iteration: gdev_pointers, mr_pr_launch.hip)
            v.v0 = 1.0 / (double)((int64_t)g->N + (int64_t)g->T);
            v.T = g->T;
            v.N = g->N;
            v.n_wt = g->n_wt;
            v.K = w.K;
            v.n_ops = w.n_ops;
            blocks.add(g->n_wt, cdiv(g->n_wt, 16), true, &v.nb, &v.per, &v.b0);
            memcpy(v.op, w.ops, (size_t)w.n_ops * sizeof(int32_t));
            KO = std::max(KO, w.n_ops);
            maxN = std::max(maxN, g->N);
        }
        const int64_t nblk = blocks.nblk;
        if (nblk >= (1ll << 31)) return mr_fail(ctx, MR_ERR_ARG, "mr_win_exemplars: too many blocks");
        DBuf<WXDev> dd;
        // ob: [nw * KO * m] score bits, then as int32 [nw * KO * m] traces, [nw * KO] counts, (dk) [nw * KO * m] class sizes
        DBuf<unsigned long long> ps, ob;
        DBuf<int32_t> pt, pk, pm;
        const size_t row = (size_t)KO * m, nm = (size_t)nw * row;
        const size_t ob_words = nm + (nm + (size_t)nw * KO + (dk ? nm : 0) + 1) / 2;
        MR_TRY(dd.upload(ctx, hd.data(), (size_t)nw));   // (hd lives until the read-back's sync below)
        MR_TRY(ps.alloc(ctx, (size_t)nblk * row));
        MR_TRY(pt.alloc(ctx, (size_t)nblk * row));
        if (dk) {
            MR_TRY(pk.alloc(ctx, (size_t)nblk * row));
            MR_TRY(pm.alloc(ctx, (size_t)nblk * row));
        }
        MR_TRY(ob.alloc(ctx, ob_words));
        const size_t dyn = ((size_t)maxN + WAVE + 15) / 16 * 16;
        hipLaunchKernelGGL(dk ? k_win_ex_select<true> : k_win_ex_select<false>, dim3((unsigned)nblk), dim3(EX_T), dyn, st,
                           (const WXDev*)dd.p, nw, KO, m, ps.p, pt.p, pk.p, pm.p);
        int32_t* ot = (int32_t*)(ob.p + nm);
        hipLaunchKernelGGL(dk ? k_win_ex_merge<true> : k_win_ex_merge<false>, dim3((unsigned)(nw * KO)), dim3(EX_T), 0, st,
                           (const WXDev*)dd.p, KO, m, (const unsigned long long*)ps.p, (const int32_t*)pt.p, ob.p, ot,
                           ot + nm, (const int32_t*)pk.p, (const int32_t*)pm.p, ot + nm + (size_t)nw * KO);
        MR_TRY_HIP(ctx, hipGetLastError());
        MR_TRY(mr_pin_ex(ctx, ob.p, ob_words, "mr_win_exemplars"));
        const double* hs = (const double*)ctx->pin_ex;
        const int32_t* hts = (const int32_t*)(ctx->pin_ex + nm);
        const int32_t* hn = hts + nm;
        const int32_t* hm = hn + (size_t)nw * KO;
        for (int i = 0; i < nw; ++i) {
            const MrWinEx& w = ws[lo[(size_t)i]];
            for (int32_t j = 0; j < w.n_ops; ++j) {
                const size_t r = (size_t)i * row + (size_t)j * m;
                memcpy(w.score + (size_t)j * m, hs + r, (size_t)m * sizeof(double));
                memcpy(w.trace + (size_t)j * m, hts + r, (size_t)m * sizeof(int32_t));
                if (dk && w.mult) memcpy(w.mult + (size_t)j * m, hm + r, (size_t)m * sizeof(int32_t));
                w.cnt[j] = hn[(size_t)i * KO + j];
            }
        }
    }
    for (int k = 0; k < n; ++k) {
        const MrWinEx& w = ws[k];
        mr_graph* g = w.g;
        if (!w.n_ops || g->lo) continue;
        if (!g->node_podop.p || !g->trace_code.p)
            return mr_fail(ctx, MR_ERR_STATE, "mr_win_exemplars: window graph without node / trace codes");
        // what the window's ranking left (the batch's asynchronous groups keep no record on the graph)
        g->rk_ok = true;
        g->rk_fp32 = w.fp32;
        g->rk_kc = false;
        g->rk_iters = w.K;
        g->rk_d = 0.85;
        g->trank_ok = false;
        std::vector<int32_t> np((size_t)g->N), tcv((size_t)g->T);
        MR_TRY(g->node_podop.download(ctx, np.data(), (size_t)g->N));
        MR_TRY(g->trace_code.download(ctx, tcv.data(), (size_t)g->T));
        MR_TRY_HIP(ctx, hipStreamSynchronize(st));
        int32_t node[EX_MAXOPS], at[EX_MAXOPS], nh = 0;
        for (int32_t j = 0; j < w.n_ops; ++j)
            for (int32_t o = 0; o < g->N; ++o)
                if (np[(size_t)o] == w.ops[j]) {
                    node[nh] = o;
                    at[nh++] = j;
                    break;
                }
        if (!nh) continue;
        std::vector<int32_t> tr((size_t)nh * m), cn((size_t)nh), mu(dk ? (size_t)nh * m : 0);
        std::vector<double> sc((size_t)nh * m);
        MR_TRY(mr_graph_exemplars_ex(g, node, nh, m, flags, tr.data(), sc.data(), cn.data(), dk ? mu.data() : nullptr));
        for (int32_t h = 0; h < nh; ++h) {
            const int32_t j = at[h];
            w.cnt[j] = cn[(size_t)h];
            for (int32_t e = 0; e < m; ++e) {
                const int32_t t = tr[(size_t)h * m + e];
                w.trace[(size_t)j * m + e] = t >= 0 ? tcv[(size_t)t] : -1;
                w.score[(size_t)j * m + e] = sc[(size_t)h * m + e];
                if (dk && w.mult) w.mult[(size_t)j * m + e] = mu[(size_t)h * m + e];
            }
        }
    }
    return MR_OK;
}
