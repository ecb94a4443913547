// The fused iteration's first half, device side: the walk kernel k_tr_a and everything only it
// inlines -- a tile's register set (TrTile), the register-accumulated hot ops (TrHot), the
// short-tile walk and the general walk (tr_walk_short, tr_walk), the call-graph terms' share
// (tr_ssv_share) and the last-block finish (tr_last_finish).  Included by mr_pr_walk.hip alone, which
// instantiates the variants; the LDS image (TrLds) and the variant bits (TR_X_*): mr_pr_walk.h.
#pragma once
#include <type_traits>

#include "mr_iter_dev.h"
#include "mr_pr_internal.h"
#include "mr_pr_walk.h"
#include "mr_prim.h"

namespace {

// ---------------------------------------------------------------- fused iteration, trace-parallel (k_tr_a)
// The single-pass iteration with lane = trace.  At prepare a graph's traces are sorted by op
// count (tperm: position -> trace) and cut into wave tiles of 64 positions; a tile stores its
// traces' ids lane-interleaved in chunks of 4 (chunk c = 64 lanes x 4 u16: one coalesced 512-B
// load), padded to the tile's longest trace with N + lane (a zero su slot and a dummy
// accumulator per lane, so pads neither branch nor collide), and each trace rotated by
// (lane mod len): a trace's first op is often a root shared by the whole tile, and rotation
// spreads those atomics over the chunk's four instructions and many lanes' addresses.
// Each wave streams a contiguous run of tiles as ONE chunk stream -- ids three chunks ahead,
// the su of cold ops (WV_SU_HOT / GLOBAL) one chunk ahead, a tile's q, (1-d) v and w one tile
// ahead -- with every load unconditional (clamped), so each use waits for exactly its own load.
// Per entry: one su read (LDS, or the prefetched gather), one add into the lane's own trace sum
// (sequential: deterministic), one LDS u64 atomic of the lane's X_t (integers: order-free).  The
// block synchronises only to clear the accumulator and to write its partial row.

// Short tiles (tiles of exactly NC chunks, NC <= 8: traces of <= 32 ops), su in LDS: a tile is ONE register
// set -- its NC id chunks, q, c = (1-d) v, w (EXT & TR_X_KINDS: the kind multiplicity's mw instead),
// the cold half of the sums (EXT & TR_X_COLD), and the chunk offsets of the next two tiles -- loaded
// unconditionally (addresses clamped) one whole tile ahead.  The tile loop is unrolled by two so
// the two register sets alternate by renaming: no register with a load in flight is ever copied,
// so the only memory waits are for loads issued a tile earlier (the ring of tr_walk's general
// loop below rotates per chunk and at tile ends has to copy the next tile's q, which made every
// tile end wait for all loads in flight, the ids three chunks ahead included).  Tiles are sorted
// by length, so a wave's run is a sequence of short-tile tiers (NC = 1, 2, .., 8, each a code copy
// with every count static) and a suffix of longer tiles the general loop takes.  Same per-lane sums
// in the same order as the general loop: bitwise equal results.
// su in k_tr_a's LDS: doubles, or 4-B floats on fp32 wide graphs (EXT & TR_X_W32: every su value of such
// a graph is rounded to float where it is made, so the float copy is exact)
template <class Q, int EXT>
using TrSu = std::conditional_t<((EXT & TR_X_W32) != 0) && std::is_same<Q, float>::value, float, double>;
template <class Q, int NC, int EXT>
struct TrTile {
    u32x2 id[NC];
    Q q;
    float c;
    float w;
    double mw;     // EXT & TR_X_KINDS: w times the kind multiplicity (kind-compressed graphs)
    u32x2 cid[2];  // EXT & TR_X_COLD: the tile's first two cold chunks (wide graphs: 2 cold labels per lane each)
    double xo;     // EXT & TR_X_COLD: k_cold_trace's sum when the tile has more cold chunks (else a dummy)
    int32_t ccw;   // EXT & TR_X_COLD: lane j: ccoff[k + 1 + j] (the next tile's cold chunk range)
    int32_t cw;    // lane j: coff[k + 1 + j] (readlane 0 / 1: the next tile's chunk range)
    uint32_t hm;   // the trace's hot-op bits (nhr > 0)
    uint32_t rl;   // the run of identical traces this lane heads (0: another lane's run; 1: its own)
    uint32_t rln;  // the next tile's rl (a tail loads nothing of its own: its loads need it a tile ahead)
    u32x2 cidn[2]; // EXT & TR_X_W32: the NEXT tile's first two cold chunks (its gathers go out a tile early)
    float cf[4];   // EXT & TR_X_W32: this tile's non-warm cold su, gathered while the previous tile walked
    float xw;      // EXT & TR_X_W32: this tile's warm cold su (LDS), summed at the previous tile's end
};
// the hot ops of a trace: their su first in the lane's sum (the same order in both walks), X into
// the lane's register accumulators (integers: order-free; flushed once per walk)
// The su part is one LDS read of hs[hm] = the sum of the trace's hot su in h order (k_tr_a builds
// the 256 sums per iteration: adding the absent ops' +0.0 would not change a sum, so hs[hm] is the
// lane's own sequential sum over its hot ops).
template <int HN>
struct TrHot {
    int32_t n;
    const double* hs;   // LDS [256]
    unsigned long long acc[HN];
};
// (every one of the HOT_MAX accumulators is updated: ops past nhr are never in a mask, so they
// add 0 -- no per-op condition, no duplicated registers)
template <int HN>
__device__ __forceinline__ double tr_hot_init(TrHot<HN>& H, uint32_t hm, unsigned long long X) {
#pragma unroll
    for (int h = 0; h < HN; ++h) {
        const unsigned long long sel = (unsigned long long)(long long)(((int32_t)(hm << (31 - h))) >> 31);
        H.acc[h] += X & sel;
    }
    return H.hs[hm];
}
// hs[m] for m = tid < 256 (su of every op in LDS; the caller synchronises before and after)
template <class SU>
__device__ __forceinline__ void tr_hot_sums(const GDev& G, const SU* su_l, double* hs, int32_t tid) {
    if (tid < 256) {
        double a = 0.0;
        for (int h = 0; h < G.nhr; ++h)
            if ((tid >> h) & 1) a += su_l[G.hop[h]];
        hs[tid] = a;
    }
}
template <class Q, int NC, int EXT, int HN>
__device__ __forceinline__ int32_t tr_walk_short(const GDev& G, int32_t k, const int32_t ke, int32_t T, int32_t lane,
                                                 int cur, int nxt, double d, double Ms, double xsc, const TrSu<Q, EXT>* su_l,
                                                 unsigned long long* lacc, double& rmax, TrHot<HN>& H, int32_t& c0,
                                                 int32_t& n, int32_t& q0, int32_t& nq) {
    const GLB int32_t* coff = gp(G.coff);
    const GLB Q* qc = gp((const Q*)G.q[cur]);
    GLB Q* qn = gpw((Q*)G.q[nxt]);
    const GLB float* c_tp = gp(G.c_tp);
    const GLB float* w_tp = gp(G.w_tp);
    // EXT: a graph of the launch may carry mw / cold sums; graphs without them load a valid dummy
    // (su[0]) and select the plain value -- unconditional loads, no branches around them
    const GLB double* sug = gp(G.sub[cur]);
    const bool kc = (EXT & TR_X_KINDS) && G.mw_tp, cx = (EXT & TR_X_COLD) && G.cold_acc;
    const GLB double* mw_tp = kc ? gp(G.mw_tp) : sug;
    // wide graphs: the cold entries' su gathered here (issued when a tile starts, summed when it
    // ends: a tile of LDS work hides the L2 latency), no cold_acc pass for these tiles
    const GLB u32x2* cids = gp((const u32x2*)G.ctids) + lane;
    const GLB int32_t* ccoff = cx ? gp(G.ccoff) : coff;
    const int32_t ccl = max(__builtin_amdgcn_readfirstlane(ccoff[ke]) - 1, 0);
    const uint32_t cpad = (uint32_t)(G.N + lane);
    // EXT & TR_X_W32: cold labels below ns_warm ("warm") read their su from LDS slot label + TR_PAD; the
    // other labels from global memory.  Both reads issue for every slot: the LDS one of a non-warm
    // label reads the lane's zero pad slot NA + lane, the global one of a warm label the lane's zero
    // pad N + lane (one coalesced line per wave) -- the sum of the two is the label's su exactly
    constexpr bool W32 = (EXT & TR_X_W32) != 0;
    const uint32_t nsw = W32 ? (uint32_t)G.ns_warm : 0u, lzero = W32 ? (uint32_t)(G.NA + lane) : 0u;
    const GLB float* sugf = W32 ? gp((const float*)G.suf[cur]) : nullptr;
    const bool hot = H.n > 0;
    const GLB uint8_t* hmk = hot ? gp(G.hmask) : (const GLB uint8_t*)coff;
    // EXT & TR_X_RUNS: run-merged graphs (trun).  Without it the run logic is compiled out: every lane walks
    // its own trace (the headline walk)
    constexpr bool RUNS = (EXT & TR_X_RUNS) != 0;
    const GLB uint8_t* trn = RUNS ? gp(G.trun) : nullptr;
    const int32_t cl = __builtin_amdgcn_readfirstlane(coff[ke]) - 1;   // the run's last chunk
    // the first tile's chunk ranges: handed over by the previous tier (n >= 0), else loaded
    if (n < 0) {
        const int32_t v = coff[min(k + lane, ke)];
        c0 = __builtin_amdgcn_readfirstlane(v);
        n = __builtin_amdgcn_readlane(v, 1) - c0;
        if constexpr ((EXT & TR_X_COLD) != 0) {
            const int32_t u = ccoff[min(k + lane, ke)];
            q0 = __builtin_amdgcn_readfirstlane(u);
            nq = __builtin_amdgcn_readlane(u, 1) - q0;
        }
    }
    if (n != NC) return k;
    using R = TrTile<Q, NC, EXT>;
    const GLB double* cacc = cx ? gp(G.cold_acc) : sug;
    // run marks of tile kk's lanes (1 on graphs without runs)
    auto rl_of = [&](int32_t kk) -> uint32_t {
        if constexpr (!RUNS) return 1u;
        return trn ? (uint32_t)trn[min(min(kk, ke - 1) * WAVE + lane, T - 1)] : 1u;
    };
    // a run's tail (rl 0) needs none of its own ids, q, c or w -- the head walks for it and its r'
    // comes by shuffle -- so its loads go to one shared word each (one cache line per load, not
    // its own): unconditional loads, no branch
    const GLB u32x2* idb = gp((const u32x2*)G.tids);
    auto load = [&](R& r, int32_t kk, int32_t cc0, int32_t qq0, int32_t nqq, uint32_t rl, int32_t qn1 = 0) {
        const int32_t kq = min(kk, ke - 1);
        const int32_t p = min(kq * WAVE + lane, T - 1);
        const bool hd = !RUNS || rl != 0u;
        const int32_t ph = hd ? p : 0;
#pragma unroll
        for (int j = 0; j < NC; ++j) r.id[j] = idb[hd ? (size_t)min(cc0 + j, cl) * WAVE + lane : 0];
        r.q = qc[ph];
        r.c = c_tp[ph];
        r.w = w_tp[ph];
        if constexpr ((EXT & TR_X_KINDS) != 0) r.mw = mw_tp[kc ? p : 0];
        if constexpr ((EXT & TR_X_COLD) != 0) {
            if (cx) {   // (uniform; ctids exists only on wide graphs)
                if constexpr (W32) {   // tile kk + 1's labels (its first cold chunk qn1)
                    r.cidn[0] = cids[(size_t)min(qn1, ccl) * WAVE];
                    r.cidn[1] = cids[(size_t)min(qn1 + 1, ccl) * WAVE];
                } else {
                    r.cid[0] = cids[(size_t)min(qq0, ccl) * WAVE];
                    r.cid[1] = cids[(size_t)min(qq0 + 1, ccl) * WAVE];
                }
            }
            r.xo = cacc[nqq > 2 ? p : 0];   // (unconditional: a branch here costs ~50 VGPRs)
            r.ccw = ccoff[min(kq + 1 + lane, ke)];
        }
        r.cw = coff[min(kq + 1 + lane, ke)];
        r.hm = hot ? hmk[p] : 0u;   // (uniform)
        r.rl = rl;
        r.rln = rl_of(kk + 1);
    };
    // tile kk from r: lane = position kk * 64 + lane
    // EXT & TR_X_W32: a tile's cold labels (l4: pads past its cold chunk count), their non-warm su gathered
    // into dst.cf (global; warm labels read the lane's zero pad) and their warm su summed into
    // dst.xw (LDS; non-warm labels read the lane's zero pad slot)
    auto labels = [&](const u32x2 (&cid)[2], int32_t nqq, uint32_t (&l4)[4]) {
        l4[0] = nqq > 0 ? cid[0].x : cpad;
        l4[1] = nqq > 0 ? cid[0].y : cpad;
        l4[2] = nqq > 1 ? cid[1].x : cpad;
        l4[3] = nqq > 1 ? cid[1].y : cpad;
    };
    auto gissue = [&](R& dst, const u32x2 (&cid)[2], int32_t nqq) {
        uint32_t l4[4];
        labels(cid, nqq, l4);
#pragma unroll
        for (int i = 0; i < 4; ++i) dst.cf[i] = sugf[l4[i] < nsw ? cpad : l4[i]];
    };
    auto wsum = [&](R& dst, const u32x2 (&cid)[2], int32_t nqq) {
        uint32_t l4[4];
        labels(cid, nqq, l4);
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) a += (float)su_l[l4[i] < nsw ? l4[i] + (uint32_t)TR_PAD : lzero];
        dst.xw = a;
    };
    // W32: nx = the next tile's register set (its gathers issued here from r.cidn, its warm sum at
    // the end), nqn = the next tile's cold chunk count
    auto run = [&](const R& r, int32_t kk, int32_t qq0, int32_t nqq, R* nx = nullptr, int32_t nqn = 0) {
        const int32_t p = kk * WAVE + lane;
        const bool own = p < T;
        double cg[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (W32)
            if (cx) gissue(*nx, r.cidn, nqn);
        if constexpr ((EXT & TR_X_COLD) != 0 && !W32)
            if (cx) {   // the first two cold chunks' su (pads past the tile's chunk count: N + lane, 0)
                const uint32_t l4[4] = {nqq > 0 ? r.cid[0].x : cpad, nqq > 0 ? r.cid[0].y : cpad,
                                        nqq > 1 ? r.cid[1].x : cpad, nqq > 1 ? r.cid[1].y : cpad};
#pragma unroll
                for (int i = 0; i < 4; ++i) cg[i] = sug[l4[i]];
            }
        // a run of rl identical traces (the same ops in the same order, the same q, c and w: the
        // same sum and r') is walked by its head alone: its X times rl into the accumulators (integers:
        // exactly the rl separate adds), its r' broadcast to the run below
        const bool hd = !RUNS || r.rl != 0u;
        const unsigned long long X0 = own && hd ? (unsigned long long)__double2ull_rn((double)r.q * xsc) : 0ull;
        const unsigned long long X = RUNS ? X0 * (unsigned long long)r.rl : X0;
        double acc = H.n ? tr_hot_init(H, r.hm, X) : 0.0;
        if (hd) {
            double sv[2][4];
            auto rd = [&](const u32x2 w, double* s) {
                s[0] = su_l[w.x & 0xffffu];
                s[1] = su_l[w.x >> 16];
                s[2] = su_l[w.y & 0xffffu];
                s[3] = su_l[w.y >> 16];
            };
            rd(r.id[0], sv[0]);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                if (j + 1 < NC) rd(r.id[j + 1], sv[(j + 1) & 1]);
                const u32x2 w = r.id[j];
                atomicAdd(&lacc[(w.x & 0xffffu)], X);
                atomicAdd(&lacc[(w.x >> 16)], X);
                atomicAdd(&lacc[(w.y & 0xffffu)], X);
                atomicAdd(&lacc[(w.y >> 16)], X);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc += sv[j & 1][i];
            }
        }
        double x = 0.0;   // the cold half, sequential in the trace's cold order (k_cold_trace's)
        if constexpr ((EXT & TR_X_COLD) != 0)
            if (cx) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x += W32 ? (double)r.cf[i] : cg[i];
                if constexpr (W32) {
                    x += (double)r.xw;   // (the warm part after the global one: a fixed order)
                    wsum(*nx, r.cidn, nqn);   // the next tile's warm sum (its labels still in r)
                }
                if (nqq > 2) x = r.xo;   // (rare: > 4 cold entries in a trace of the tile: k_cold_trace's sum)
            }
        double rp = d * ((acc + x) / Ms) + (double)r.c;   // pagerank.py:125
        if (RUNS && trn) {   // (uniform) the run's head's r'
            const unsigned long long hb = __ballot(hd) & (lane == WAVE - 1 ? ~0ull : (2ull << lane) - 1ull);
            rp = __shfl(rp, 63 - __builtin_clzll(hb), WAVE);
        }
        if (own) rmax = nmax(rmax, rp);
        const double wq = kc ? r.mw : (double)r.w;
        qn[own && hd ? p : T] = (Q)(wq * rp);   // q[T]: pad slot (a run's tails never read theirs)
    };
    R A, B;
    if constexpr (W32) {
        // the tier's first tile: its cold labels and gathers here (later tiles' go out a tile early),
        // the next tile's cold range from lanes 1 and 2 of the cold offsets
        const int32_t u3 = ccoff[min(k + lane, ke)];
        const int32_t q1 = __builtin_amdgcn_readlane(u3, 1), nq1 = __builtin_amdgcn_readlane(u3, 2) - q1;
        u32x2 c0v[2];
        c0v[0] = cids[(size_t)min(q0, ccl) * WAVE];
        c0v[1] = cids[(size_t)min(q0 + 1, ccl) * WAVE];
        if (cx) {
            gissue(A, c0v, nq);
            wsum(A, c0v, nq);
        }
        load(A, k, c0, q0, nq, rl_of(k), q1);
        int32_t nqA1 = nq1;   // tile k + 1's cold chunk count
        for (;;) {
            const int32_t c0B = __builtin_amdgcn_readfirstlane(A.cw);
            const int32_t nB = __builtin_amdgcn_readlane(A.cw, 1) - c0B;
            const int32_t qB = __builtin_amdgcn_readfirstlane(A.ccw);
            const int32_t nqB = __builtin_amdgcn_readlane(A.ccw, 1) - qB;
            const int32_t qB1 = __builtin_amdgcn_readlane(A.ccw, 1), nqB1 = __builtin_amdgcn_readlane(A.ccw, 2) - qB1;
            load(B, k + 1, c0B, qB, nqB, A.rln, qB1);
            run(A, k, q0, nq, &B, nqA1);
            if (++k == ke || nB != NC) {
                c0 = c0B, n = nB, q0 = qB, nq = nqB;
                break;
            }
            const int32_t c0A = __builtin_amdgcn_readfirstlane(B.cw);
            const int32_t nA2 = __builtin_amdgcn_readlane(B.cw, 1) - c0A;
            const int32_t qA2 = __builtin_amdgcn_readfirstlane(B.ccw);
            const int32_t nqA2 = __builtin_amdgcn_readlane(B.ccw, 1) - qA2;
            const int32_t qA1 = __builtin_amdgcn_readlane(B.ccw, 1);
            nqA1 = __builtin_amdgcn_readlane(B.ccw, 2) - qA1;
            load(A, k + 1, c0A, qA2, nqA2, B.rln, qA1);
            run(B, k, qB, nqB, &A, nqB1);
            if (++k == ke || nA2 != NC) {
                c0 = c0A, n = nA2, q0 = qA2, nq = nqA2;
                break;
            }
            q0 = qA2, nq = nqA2;
        }
        return k;
    }
    load(A, k, c0, q0, nq, rl_of(k));
    int32_t nA = n, qA = q0, nqA = nq;
    for (;;) {
        // B = tile k + 1 (its ranges from A's offsets), then A's tile
        const int32_t c0B = __builtin_amdgcn_readfirstlane(A.cw);
        const int32_t nB = __builtin_amdgcn_readlane(A.cw, 1) - c0B;
        int32_t qB = 0, nqB = 0;
        if constexpr ((EXT & TR_X_COLD) != 0) {
            qB = __builtin_amdgcn_readfirstlane(A.ccw);
            nqB = __builtin_amdgcn_readlane(A.ccw, 1) - qB;
        }
        load(B, k + 1, c0B, qB, nqB, A.rln);
        run(A, k, qA, nqA);
        if (++k == ke || nB != NC) {
            c0 = c0B, n = nB, q0 = qB, nq = nqB;
            break;
        }
        const int32_t c0A = __builtin_amdgcn_readfirstlane(B.cw);
        nA = __builtin_amdgcn_readlane(B.cw, 1) - c0A;
        if constexpr ((EXT & TR_X_COLD) != 0) {
            qA = __builtin_amdgcn_readfirstlane(B.ccw);
            nqA = __builtin_amdgcn_readlane(B.ccw, 1) - qA;
        }
        load(A, k + 1, c0A, qA, nqA, B.rln);
        run(B, k, qB, nqB);
        if (++k == ke || nA != NC) {
            c0 = c0A, n = nA, q0 = qA, nq = nqA;
            break;
        }
    }
    return k;
}

// The wave's walk of k_tr_a over its run of wave tiles: per entry one
// su read, one add into the lane's trace sum, one LDS u64 atomic of X_t; per tile r' of its traces
// and their next q.  Returns the wave's largest r' (-inf when it owns no trace).
template <class Q, int SUM, int NT, int EXT = 0, bool HOTT = false>
__device__ __forceinline__ double tr_walk(const GDev& G, int32_t lb, int cur, int nxt, int32_t N, int32_t NH, double d,
                                          double Ms, double xsc, const TrSu<Q, EXT>* su_l, unsigned long long* lacc,
                                          const double* hs = nullptr) {
    constexpr bool SUL = SUM == WV_SU_ALL, HOT = SUM == WV_SU_HOT;
    constexpr int NW = NT / WAVE;
    const int32_t T = G.T;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const GLB u32x2* ids = gp((const u32x2*)G.tids) + lane;   // chunk c of this lane: ids[c * WAVE]
    const GLB int32_t* coff = gp(G.coff);
    const GLB Q* qc = gp((const Q*)G.q[cur]);
    GLB Q* qn = gpw((Q*)G.q[nxt]);
    const GLB float* c_tp = gp(G.c_tp);
    const GLB float* w_tp = gp(G.w_tp);
    const GLB double* sug = gp(G.sub[cur]);   // ids >= N are pads (su 0)
    // this wave's tiles [k, ke) (a contiguous run: the host cuts them by chunk count)
    const GLB int32_t* wt = gp(G.wtile) + ((size_t)lb * NW + wv);
    int32_t k = __builtin_amdgcn_readfirstlane(wt[0]);
    const int32_t ke = __builtin_amdgcn_readfirstlane(wt[1]);
    double rmax = -__builtin_huge_val();
    constexpr int HN = (EXT & TR_X_COLD) ? HOT_MAX_WIDE : HOT_MAX;
    TrHot<HN> H;
    H.n = SUL && HOTT ? __builtin_amdgcn_readfirstlane(G.nhr) : 0;   // (the host strips only such graphs)
    H.hs = hs;
#pragma unroll
    for (int h = 0; h < HN; ++h) H.acc[h] = 0ull;
    const int32_t k_first = k;
    if constexpr (SUL) {
        // one tier per chunk count (the run's tiles ascend in it): every count static, no branch
        // inside a tile, so each wait is for exactly the LDS reads and loads it consumes
        int32_t tc0 = 0, tn = -1, tq0 = 0, tnq = 0;   // the next tile's ranges, handed from tier to tier
#define TR_TIER(NC_) if (NC_ <= ((EXT & TR_X_W32) ? TR_TIERS_W32 : NT == 1024 || (EXT & (TR_X_KINDS | TR_X_COLD)) ? TR_TIERS_EXT : MR_TR_TIERS512) && k < ke) k = tr_walk_short<Q, NC_, EXT, HN>(G, k, ke, T, lane, cur, nxt, d, Ms, xsc, su_l, lacc, rmax, H, tc0, tn, tq0, tnq);
        TR_TIER(1) TR_TIER(2) TR_TIER(3) TR_TIER(4) TR_TIER(5) TR_TIER(6) TR_TIER(7) TR_TIER(8)
#undef TR_TIER
    }
    const GLB uint8_t* hmk = gp(G.hmask);
    if (k < ke) {
        auto pos = [&](int32_t kk) { return min(kk * WAVE + lane, T - 1); };
        // cold-op su of a chunk (LDS-resident ops load sug[0]: one line, no traffic; pads read as 0)
        auto gather = [&](const u32x2 w, double* g) {
            const int32_t o[4] = {(int32_t)(w.x & 0xffffu), (int32_t)(w.x >> 16), (int32_t)(w.y & 0xffffu),
                                  (int32_t)(w.y >> 16)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double v = SUL ? 0.0 : sug[HOT && o[j] < NH ? 0 : min(o[j], N - 1)];
                g[j] = o[j] < N ? v : 0.0;
            }
        };
        int32_t c = __builtin_amdgcn_readfirstlane(coff[k]);
        int32_t ce = __builtin_amdgcn_readfirstlane(coff[k + 1]);   // end of tile k
        const int32_t cl = __builtin_amdgcn_readfirstlane(coff[ke]) - 1;   // the run's last chunk
        // tile k's words; tile k + 1's q and end chunk (one tile ahead, clamped into the run).  The
        // end chunk is loaded per lane (lane-varying address: a vector load -- a scalar load would
        // share lgkmcnt with the LDS traffic and force full drains)
        const int32_t kn = min(k + 1, ke - 1);
        // w_t of a position: times the kind's multiplicity on a kind-compressed graph (uniform branch)
        const GLB double* mw_tp = gp(G.mw_tp);
        auto wq = [&](int32_t kk) { return mw_tp ? mw_tp[pos(kk)] : (double)w_tp[pos(kk)]; };
        double q_cur = (double)qc[pos(k)];
        float c_cur = c_tp[pos(k)];
        // wide graphs: the cold half of the trace's sum (k_cold_trace), else 0 (acc + 0 = acc)
        const GLB double* cacc = gp(G.cold_acc);
        double x_cur = cacc ? cacc[pos(k)] : 0.0;
        double w_cur = wq(k);
        double q_nx = (double)qc[pos(kn)];
        int32_t ce_nx = coff[min(kn + 1 + lane, ke)];
        // su of a chunk's ops from LDS (HOT: the hot part; the cold part comes from gather)
        auto lds_su = [&](const u32x2 w, double* sv) {
            const int32_t o[4] = {(int32_t)(w.x & 0xffffu), (int32_t)(w.x >> 16), (int32_t)(w.y & 0xffffu),
                                  (int32_t)(w.y >> 16)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sv[j] = SUL ? su_l[o[j]] : HOT ? su_l[min(o[j], NH - 1)] : 0.0;
            }
        };
        // ids ring (4 chunks: the current one and three ahead), su ping-pong (current, next)
        u32x2 wa = ids[(size_t)c * WAVE];
        u32x2 wb = ids[(size_t)min(c + 1, cl) * WAVE];
        u32x2 wc = ids[(size_t)min(c + 2, cl) * WAVE];
        u32x2 wd;
        double gA[4], gB[4], sA[4], sB[4];
        if (!SUL) gather(wa, gA);
        if (SUL || HOT) lds_su(wa, sA);
        unsigned long long X = k * WAVE + lane < T ? (unsigned long long)__double2ull_rn(q_cur * xsc) : 0ull;
        double acc = H.n ? tr_hot_init(H, hmk[pos(k)], X) : 0.0;
        // One chunk: ids CUR (here), su SC / GC (LDS here, cold gathers in flight); NXT's cold
        // gathers and LDS reads go out before CUR's atomics (their latency, bank conflicts
        // included, overlaps a whole chunk), and the ids three chunks ahead land in LD.  The loop
        // is unrolled 4x so the ring rotates by renaming, not by register moves (a move of an
        // in-flight register would wait for it).
#define TR_STEP(CUR, NXT, LD, GC, SC, GN, SN)                                                              \
        {                                                                                                  \
            LD = ids[(size_t)min(c + 3, cl) * WAVE];                                                       \
            if (!SUL) gather(NXT, GN);                                                                     \
            if (SUL || HOT) lds_su(NXT, SN);                                                               \
            const int32_t o_[4] = {(int32_t)(CUR.x & 0xffffu), (int32_t)(CUR.x >> 16),                     \
                                   (int32_t)(CUR.y & 0xffffu), (int32_t)(CUR.y >> 16)};                    \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) atomicAdd(&lacc[o_[j]], X);                         \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                  \
                acc += SUL ? SC[j] : HOT ? (o_[j] < NH ? SC[j] : GC[j]) : GC[j];                          \
            if (++c == ce) {                                                                               \
                /* tile k done: r' of its traces (pagerank.py:125) and the next q */                      \
                const int32_t p_ = k * WAVE + lane;                                                        \
                const bool own_ = p_ < T;                                                                  \
                const double rp_ = d * ((acc + x_cur) / Ms) + (double)c_cur;                               \
                if (own_) rmax = nmax(rmax, rp_);                                                          \
                qn[own_ ? p_ : T] = (Q)(w_cur * rp_);   /* q[T]: pad slot */                              \
                if (++k == ke) goto tr_done;                                                               \
                ce = __builtin_amdgcn_readfirstlane(ce_nx);                                                \
                q_cur = q_nx;                                                                              \
                const int32_t kk_ = min(k + 1, ke - 1);                                                    \
                c_cur = c_tp[pos(k)];                                                                      \
                x_cur = cacc ? cacc[pos(k)] : 0.0;                                                         \
                w_cur = wq(k);                                                                             \
                q_nx = (double)qc[pos(kk_)];                                                               \
                ce_nx = coff[min(kk_ + 1 + lane, ke)];                                                     \
                X = p_ + WAVE < T ? (unsigned long long)__double2ull_rn(q_cur * xsc) : 0ull;               \
                acc = H.n ? tr_hot_init(H, hmk[pos(k)], X) : 0.0;                                          \
            }                                                                                              \
        }
        for (;;) {
            TR_STEP(wa, wb, wd, gA, sA, gB, sB)
            TR_STEP(wb, wc, wa, gB, sB, gA, sA)
            TR_STEP(wc, wd, wb, gA, sA, gB, sB)
            TR_STEP(wd, wa, wc, gB, sB, gA, sA)
        }
#undef TR_STEP
    tr_done:;
    }
    // the hot ops' accumulators: a wave sum each (integers), one LDS add
    if (k_first < ke)
#pragma unroll
        for (int h = 0; h < HN; ++h)
            if (h < H.n) {
                unsigned long long a = H.acc[h];
#pragma unroll
                for (int m = WAVE / 2; m >= 1; m >>= 1) a += (unsigned long long)__shfl_xor((long long)a, m, WAVE);
                if (lane == 0) atomicAdd(&lacc[G.hop[h]], a);
            }
    return rmax;
}

// The call-graph term alpha (P_ss s_k)[o] / M_s(k) of k_fx_b (pagerank.py:122-124), computed in
// k_tr_a instead: block lb owns the columns [lb N / n_fa, (lb + 1) N / n_fa), and every wave that
// has finished its walk takes chunks of 64 of them (an LDS counter) -- the chains of dependent
// loads (ss_off -> ss_par -> pw, s_k) then run in the slack of the block's slowest wave, not in
// k_fx_b's critical path.  The same arithmetic as k_fx_b (a lane per column of <= 8 parents with
// wave_sum's butterfly value, a wave per column of more): fx_ssv[o], read there bitwise.
// (pf: s_k from the block's LDS copy spl -- this launch computed it -- and the terms into buffer
// it & 1 of fx_ssv, read by the next launch's prologue or the final k_fx_b)
__device__ __forceinline__ void tr_ssv_share(const GDev& G, int32_t lb, int cur, double Ms, int* ctr, int lane,
                                             const double* spl = nullptr, int64_t ssv_off = 0) {
    const int32_t N = G.N;
    const int32_t oa = (int32_t)((int64_t)lb * N / G.n_fa), ob = (int32_t)((int64_t)(lb + 1) * N / G.n_fa);
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(ctr, WAVE);
        c = __builtin_amdgcn_readfirstlane(c);
        if (oa + c >= ob) return;
        const int32_t o = oa + c + lane;
        const bool on = o < ob;
        const int32_t op = on && G.perm ? G.perm[o] : o;
        const GLB int64_t* ss_off = gp(G.ss_off);
        const GLB int32_t* ss_par = gp(G.ss_par);
        const GLB float* pw = gp(G.pw);
        const GLB double* spg = gp(G.spb[cur]);
        auto sp = [&](int32_t p) -> double { return spl ? spl[p] : spg[p]; };
        double ssv = 0.0;
        bool big = false;
        if (on) {
            const int64_t e0 = ss_off[op], e1 = ss_off[op + 1];
            if (e1 - e0 <= 8) {
                int32_t pp[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) pp[k] = e0 + k < e1 ? ss_par[e0 + k] : -1;
                double t[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = pp[k] >= 0 ? (double)pw[pp[k]] * sp(pp[k]) : 0.0;
                const double bb = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
                ssv = G.alpha * (bb / Ms);
            } else {
                big = true;
            }
        }
        for (uint64_t bm = __ballot(big); bm; bm &= bm - 1) {   // (wave-uniform)
            const int j = __ffsll((unsigned long long)bm) - 1;
            const int32_t opj = G.perm ? G.perm[oa + c + j] : oa + c + j;
            const int64_t e0 = ss_off[opj], e1 = ss_off[opj + 1];
            double bb = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += WAVE) {
                const int32_t pp = ss_par[e];
                bb += (double)pw[pp] * sp(pp);
            }
            bb = wave_sum(bb);
            if (lane == j) ssv = G.alpha * (bb / Ms);
        }
        if (on) {
            if (G.lastfin)   // (write-through: the graph's last block reads it with sc1 loads)
                __hip_atomic_store(gpw((unsigned long long*)G.fx_ssv) + o, (unsigned long long)__double_as_longlong(ssv),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                G.fx_ssv[ssv_off + o] = ssv;
        }
    }
}

// The last k_tr_a block of a graph finishes the iteration itself (small graphs: window batches),
// so an iteration is ONE launch instead of k_tr_a + k_fx_b.  Every block writes its partial row
// and its call-graph terms write-through (sc1, hipMalloc'd pool memory), every wave waits for its
// stores (vmcnt(0)), and behind a workgroup barrier one lane takes a ticket from the graph's
// counter (an agent-scope add, returned); the block whose ticket completes the iteration's count is
// the consumer: it reads every row and does k_fx_b's work for every op -- the same exact limb sums,
// the same call-graph term (a lane per op of <= 8 parents, a wave per op of more: wave_sum's
// butterfly) and the same finish: bitwise k_fx_b's results.  Two forms of the hand-off
// (MI355X_MICROARCH.md, inter-workgroup visibility):
//  * a launch of at most one block per CU (<= num_cus blocks, the dynamic LDS padded past half a
//    CU's 160 KB so no two blocks share a CU: single windows) is the hand-off table's row 1 in
//    every cell -- one lane per storing workgroup adds to ONE unsharded counter, the last adder
//    told by the returned value, the other waves behind a barrier it joins, hipMalloc, one
//    workgroup per CU, 8-B sc1 stores and sc1 loads: no acquire (lf_acq 0);
//  * any other launch (batches: several workgroups per CU) takes the guide's general consumer
//    form: ONE agent acquire on the adding lane, its own vmcnt(0) wait, a workgroup barrier, then
//    the loads (lf_acq 1).  Only the finishing block pays it.
template <int NT>
__device__ __forceinline__ void tr_last_finish(const GDev& G, int it, double d, double Ms,
                                            GLB unsigned long long* Mnext) {
    constexpr int NW = NT / WAVE;
    __shared__ int s_last;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave's row stores are out
    __syncthreads();
    if (tid == 0) {
        const unsigned long long t = __hip_atomic_fetch_add(gpw(G.mslot) + 6 * MSH + 1, 1ull, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t + 1 == (unsigned long long)G.n_fa * (unsigned long long)(it + 1);
        if (last && G.lf_acq) {   // consumer: agent acquire (this CU's L1 invalidated), waited before the barrier
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    const int32_t N = G.N, nb = G.n_fa, nxt = (it & 1) ^ 1;
    const GLB unsigned long long* rows = gp((const unsigned long long*)G.fx_part);
    const GLB double* sp_cur = gp(G.spb[it & 1]);
    const GLB int64_t* ss_off = gp(G.ss_off);
    const GLB int32_t* ss_par = gp(G.ss_par);
    const GLB float* pw = gp(G.pw);
    const GLB float* u_o = gp(G.u_o);
    const double iscale = G.dscale ? G.dscale[1] : G.fx_iscale;
    for (int32_t ob = wv * WAVE; ob < N; ob += NW * WAVE) {   // lane = op
        const int32_t o = ob + lane;
        const bool on = o < N;
        unsigned long long lo = 0ull, hi = 0ull;
        // 16 rows per batch, every load in flight before the sums (indices clamped; repeats not added)
        const int32_t oc = on ? o : N - 1;
        for (int32_t b0 = 0; b0 < nb; b0 += 16) {
            unsigned long long v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                v[k] = __hip_atomic_load(rows + (size_t)min(b0 + k, nb - 1) * N + oc, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (b0 + k < nb) {
                    lo += v[k] & 0xffffffffull;
                    hi += v[k] >> 32;
                }
        }
        double ssv = 0.0;
        bool big = false;
        if (on && G.ssv_pre) {   // every block computed its share of the terms (tr_ssv_share): one load
            ssv = __longlong_as_double((long long)__hip_atomic_load(gp((const unsigned long long*)G.fx_ssv) + o,
                                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        } else if (on) {
            const int64_t e0 = ss_off[o], e1 = ss_off[o + 1];
            if (e1 - e0 <= 8) {
                int32_t pp[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) pp[k] = e0 + k < e1 ? ss_par[e0 + k] : -1;
                double t[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = pp[k] >= 0 ? (double)pw[pp[k]] * sp_cur[pp[k]] : 0.0;
                const double bb = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
                ssv = G.alpha * (bb / Ms);
            } else {
                big = true;
            }
        }
        for (uint64_t bm = __ballot(big); bm; bm &= bm - 1) {   // (wave-uniform)
            const int j = __ffsll((unsigned long long)bm) - 1;
            const int32_t oj = ob + j;
            const int64_t e0 = ss_off[oj], e1 = ss_off[oj + 1];
            double bb = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += WAVE) {
                const int32_t pp = ss_par[e];
                bb += (double)pw[pp] * sp_cur[pp];
            }
            bb = wave_sum(bb);
            if (lane == j) ssv = G.alpha * (bb / Ms);
        }
        if (on) {
            const double sum = ((double)hi * 4294967296.0 + (double)lo) * iscale;
            const double v = d * (sum + ssv);   // pagerank.py:122-124
            G.spb[nxt][o] = v;
            G.sub[nxt][o] = (double)u_o[o] * v;
            atomicMax((unsigned long long*)&Mnext[o % MSH], d2bits(v));
        }
    }
}

#ifndef MR_TR_WPE512
#define MR_TR_WPE512 8   // minimum waves per SIMD asked of the plain 512-thread k_tr_a (A/B builds: 1)
#endif
template <class Q, int SUM, int NT, int EXT>
__global__ void __launch_bounds__(NT, NT == 512 && EXT == 0 && SUM != WV_SU_HOT ? MR_TR_WPE512 : 1) k_tr_a(const GDev* __restrict__ gs, int32_t ng, int32_t split, double d,
                                             double alpha, int it, int32_t unused) {
    constexpr bool SUL = SUM == WV_SU_ALL, HOT = SUM == WV_SU_HOT;
    constexpr int NW = NT / WAVE;
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    __shared__ double red[NW];
    __shared__ double msh[2];
    const GDev& G = gs[fx_graph<&GDev::blk0f>(gs, ng, split)];
    const int32_t lb = (int32_t)blockIdx.x - G.blk0f;
    const int cur = it & 1, nxt = cur ^ 1, k3 = it % 3;
    const int32_t N = G.NA;   // (wide graphs: the hot ops)
    const int32_t tid = (int32_t)threadIdx.x;
    // pf (window batches, 512-thread variant): k_fx_b's finish of the previous iteration runs here,
    // in every block of the graph (below), so an iteration is one launch
    const bool pf = NT == 512 && SUL && EXT == 0 && G.pf;
    constexpr bool W32 = (EXT & TR_X_W32) != 0;   // (fp32 wide graphs: float su, warm labels in LDS)
    using SU = TrSu<Q, EXT>;
    const TrLds L_(N, SUM, pf, W32);
    const int32_t NH = HOT ? G.n_hot : 0;   // <= L_.n_hot (the host sizes both alike), >= 64
    const GLB double* sug = gp(G.sub[cur]);   // ids >= N are pads (su 0)
    SU* su_l = (SU*)(lraw + L_.su);
    double* sp_l = (double*)(lraw + L_.sp);   // (pf) s_it itself, for the call-graph terms
    unsigned long long* lacc = (unsigned long long*)(lraw + L_.lacc);
    GLB unsigned long long* mslot = gpw(G.mslot);
    GLB unsigned long long* Mcur = mslot + (size_t)2 * MSH * k3;
    GLB unsigned long long* Mnext = mslot + (size_t)2 * MSH * ((k3 + 1) % 3);
    if (lb == 0 && tid < 2 * MSH) mslot[(size_t)2 * MSH * ((k3 + 2) % 3) + tid] = 0ull;
    double pf_max = -__builtin_huge_val();
    if (pf && it > 0) {
        // s_it[o] = d (S_o 2^-SC + alpha (P_ss s_{it-1})[o] / M_s(it-1)) from the previous launch's
        // partial rows and call-graph terms (buffers (it - 1) & 1): k_fx_b's exact limb sums and its
        // expression, so bitwise k_fx_b's values; every block of the graph computes all N of them
        // (a few rows each) -- block 0 also publishes s_it and M_s(it) for the final k_fx_b
        const int pb = (it - 1) & 1;
        const GLB unsigned long long* rows = gp((const unsigned long long*)G.fx_part) + (size_t)pb * G.pf_stride;
        const GLB double* ssvp = gp(G.fx_ssv) + (size_t)pb * N;
        const GLB float* u_o = gp(G.u_o);
        const double iscale = G.dscale ? G.dscale[1] : G.fx_iscale;
        const int32_t nb = G.n_fa;
        GLB double* spo = gpw(G.spb[cur]);
        for (int32_t o = tid; o < N + TR_PAD; o += NT) {
            if (o < N) {
                unsigned long long lo = 0ull, hi = 0ull;
                for (int32_t b = 0; b < nb; ++b) {
                    const unsigned long long v = rows[(size_t)b * N + o];
                    lo += v & 0xffffffffull;
                    hi += v >> 32;
                }
                const double sum = ((double)hi * 4294967296.0 + (double)lo) * iscale;
                const double v = d * (sum + ssvp[o]);   // pagerank.py:122-124
                sp_l[o] = v;
                su_l[o] = (double)u_o[o] * v;
                pf_max = nmax(pf_max, v);
                if (lb == 0) {
                    spo[o] = v;
                    atomicMax((unsigned long long*)&Mcur[o % MSH], d2bits(v));
                }
            } else {
                su_l[o] = 0.0;
                sp_l[o] = 0.0;
            }
        }
    } else if (W32) {   // hot ops, 64 zero pads, then the warm labels N .. ns_warm - 1
        const int32_t nw = G.ns_warm - N;
        for (int32_t o = tid; o < N + TR_PAD + nw; o += NT)
            su_l[o] = (SU)(o < N ? sug[o] : o < N + TR_PAD ? 0.0 : sug[o - TR_PAD]);
    } else if (SUL) {
        for (int32_t o = tid; o < N + TR_PAD; o += NT) su_l[o] = o < N ? sug[o] : 0.0;
        if (pf)
            for (int32_t o = tid; o < N + TR_PAD; o += NT) sp_l[o] = o < N ? G.spb[cur][o] : 0.0;
    }
    for (int32_t o = tid; o < N + TR_PAD; o += NT) lacc[o] = 0ull;
    if (HOT)
        for (int32_t o = tid; o < NH; o += NT) su_l[o] = sug[o];
    __shared__ int s_ssv;   // the call-graph term chunks taken (G.ssv_pre)
    if (tid < WAVE) {
        const double ms = wave_max(bits2d(Mcur[tid]));
        const double mr = wave_max(bits2d(Mcur[MSH + tid]));
        if (tid == 0) {
            msh[0] = ms;
            msh[1] = mr;
            s_ssv = 0;
        }
    }
    __syncthreads();   // accumulator and maxima ready
    if (pf && it > 0) {   // M_s(it): the maximum of the s_it just computed (block_max synchronises)
        const double m = block_max(pf_max, red);
        if (tid == 0) msh[0] = m;
        __syncthreads();
    }
    // hot ops (large graphs: the 1024-thread variant only) -- the mask sums of this iteration's su
    constexpr bool HOTT = SUL && NT == 1024;
    double* hs = (double*)(lraw + L_.hs);
    if (HOTT && L_.hot_ok && G.nhr) {
        tr_hot_sums(G, su_l, hs, tid);
        __syncthreads();
    }
    const double xsc = (G.dscale ? G.dscale[0] : G.fx_scale) / msh[1], Ms = msh[0];
    const double rmax_w = tr_walk<Q, SUM, NT, EXT, HOTT>(G, lb, cur, nxt, N, NH, d, Ms, xsc, su_l, lacc, hs);
    // the call-graph terms of this block's share of the columns, by the waves done walking
    if (G.ssv_pre) tr_ssv_share(G, lb, cur, Ms, &s_ssv, tid & (WAVE - 1), pf ? sp_l : nullptr, pf ? (int64_t)cur * N : 0);
    __syncthreads();
    GLB unsigned long long* prow = gpw(G.fx_part) + (pf ? (size_t)cur * G.pf_stride : 0) + (size_t)lb * N;
    if constexpr (NT == 512) {   // (window-graph variant only: the large graphs' kernel stays as it is)
        if (G.lastfin) {
            for (int32_t o = tid; o < N; o += NT)   // write-through: the last block reads them with sc1 loads
                __hip_atomic_store(prow + o, lacc[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double rmax = block_max(rmax_w, red);
            if (tid == 0 && rmax >= 0.0) atomicMax((unsigned long long*)&Mnext[MSH + blockIdx.x % MSH], d2bits(rmax));
            tr_last_finish<NT>(G, it, d, Ms, Mnext);
            return;
        }
    }
    if (G.row_wt)   // write-through (sc1): the boundary to k_fx_b has no dirty lines to write back
        for (int32_t o = tid; o < N; o += NT)
            __hip_atomic_store(prow + o, lacc[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        for (int32_t o = tid; o < N; o += NT) prow[o] = lacc[o];
    const double rmax = block_max(rmax_w, red);
    if (tid == 0 && rmax >= 0.0)   // -inf: a block without traces (an empty shard's placeholder)
        atomicMax((unsigned long long*)&Mnext[MSH + blockIdx.x % MSH], d2bits(rmax));
}

}  // namespace
