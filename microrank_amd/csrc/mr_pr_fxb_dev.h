// The fused iteration's second half, device side: k_fx_b, the column sums of k_tr_a's partial rows
// (and a wide graph's cold rows), the call-graph term and the finish of s', with a sharded graph's
// exchange in its modes 1 and 2.  Included by mr_pr_fxb.hip alone (fx_b_kernel hands it to iterate).
#pragma once
#include "mr_iter_dev.h"
#include "mr_prim.h"

namespace {

// Column sums of the partial rows: a block per chunk of FB_OPS consecutive ops (lane = op, so
// every row read is one coalesced 512-B segment), its FB_W waves splitting the rows; the waves'
// limb sums meet in LDS (integers: order-free).  mode 0: whole graph; sharded graphs split it
// around the limb all-reduce: mode 1 writes this rank's limbs (lo, hi) per op to fx_limb, mode 2
// finishes from the reduced limbs.
// (FB_W, the waves per block, and the host rule for it: mr_pr_iter.h)
// px.peers (sharded graphs on the peer path, one graph per launch): the exchange is fused in --
// mode 1 pushes the block's limbs (and block 0 this rank's r' maximum) into every rank's slot for
// this rank and stores the round number in the block's flag there; mode 2 block b waits for flag
// (src, b) of every source (px.spin; else k_peer_bwait waited before the launch) and sums the R
// slots in rank order.  Bitwise the all-reduce path: the same integers summed.
template <int FB_W>
__global__ void __launch_bounds__(WAVE * FB_W) k_fx_b(const GDev* __restrict__ gs, int32_t ng, int32_t split,
                                                     double d, int it, int mode, const MrPeerX px) {
    __shared__ unsigned long long slo[FB_W * WAVE], shi[FB_W * WAVE];
    __shared__ double lssv[WAVE];
    __shared__ int s_ok;
    const GDev& G = gs[fx_graph<&GDev::blk0fb>(gs, ng, split)];
    const bool pxo = px.peers != nullptr;   // (uniform)
    const GLB unsigned long long* preg = (const GLB unsigned long long*)px.region;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int32_t OPB = G.fb_ops, GR = WAVE / OPB;
    const int32_t ol = lane % OPB, grp = lane / OPB;
    // o: the column (the fused kernel's op label); op: the graph's op (perm: relabelled graphs)
    const int32_t o0 = ((int32_t)blockIdx.x - G.blk0fb) * OPB;
    const int32_t o = o0 + ol;
    const int32_t N = G.N, nb = G.n_fa;
    const bool on = o < N;
    const int k3c = it % 3;
    // the op's rows: k_tr_a's (stride NA), or on a wide graph its cold range's (stride cold_rw).
    // The first batch of 16 rows per lane is issued before the call-graph term below, so the two
    // chains of dependent loads overlap (window graphs: tens of rows, one batch covers them)
    const int32_t stride = FB_W * GR;
    const GLB unsigned long long* col = gp((const unsigned long long*)G.fx_part);
    int32_t nbl = 0;
    size_t rs = 1;
    if (on && mode != 2) {
        if (o < G.NA) {   // (pf graphs: the final iteration's rows, buffer it & 1)
            col = gp((const unsigned long long*)G.fx_part) + (G.pf ? (size_t)(it & 1) * G.pf_stride : 0) + o;
            nbl = nb;
            rs = (size_t)G.NA;
        } else {
            const int32_t oc = o - G.NA, r = oc / G.cold_rw, rb0 = G.cold_rowbase[r];
            nbl = G.cold_rowbase[r + 1] - rb0;
            col = gp(G.cold_part) + (size_t)rb0 * G.cold_rw + (oc - r * G.cold_rw);
            rs = (size_t)G.cold_rw;
        }
    }
    const int32_t rfirst = w * GR + grp;
    unsigned long long v0[16];
    if (nbl > 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) v0[k] = col[(size_t)min(rfirst + k * stride, nbl - 1) * rs];
    }
    // the call-graph term alpha (P_ss s_k)[op] / M_s(k) (pagerank.py:122-124) of the block's ops: a
    // wave per op, its lanes striding the op's parents, one fixed-order wave sum (a hub op with
    // thousands of parents costs one wave, not one thread).  (Not in mode 1: its sums only.)
    // ssv_pre: k_tr_a computed them (tr_ssv_share) -- one coalesced load
    if (mode != 1 && G.ssv_pre) {
        if (threadIdx.x < (unsigned)OPB)
            lssv[threadIdx.x] = o0 + (int32_t)threadIdx.x < N ? G.fx_ssv[(G.pf ? (size_t)(it & 1) * N : 0) + o0 + threadIdx.x] : 0.0;
    } else if (mode != 1) {
        const double Ms = wave_max(bits2d(G.mslot[(size_t)2 * MSH * k3c + lane]));
        const GLB double* sp_cur = gp(G.spb[it & 1]);
        const GLB int64_t* ss_off = gp(G.ss_off);
        const GLB int32_t* ss_par = gp(G.ss_par);
        const GLB float* pw = gp(G.pw);
        // the wave's ops j = w, w + FB_W, ..: one lane each for ops of <= 8 parents -- the lane
        // forms the wave sum's value itself (the butterfly of wave_sum over 64 slots with the
        // terms in slots 0..7 and zeros elsewhere: adding +0.0 is exact, so only the pairs
        // (l, l+4), (l, l+2), (0, 1) round) -- all the wave's ops in one chain of loads instead
        // of one chain per op; ops with more parents take the wave path after them
        const int32_t nj = (OPB - w + FB_W - 1) / FB_W;
        bool big = false;
        if (lane < nj) {
            const int32_t j = w + lane * FB_W, oj = o0 + j;
            if (oj < N) {
                const int32_t opj = G.perm ? G.perm[oj] : oj;
                const int64_t e0 = ss_off[opj], e1 = ss_off[opj + 1];
                if (e1 - e0 <= 8) {
                    int32_t pp[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) pp[k] = e0 + k < e1 ? ss_par[e0 + k] : -1;
                    double t[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) t[k] = pp[k] >= 0 ? (double)pw[pp[k]] * sp_cur[pp[k]] : 0.0;
                    const double bb = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
                    lssv[j] = G.alpha * (bb / Ms);
                } else {
                    big = true;
                }
            }
        }
        for (uint64_t bm = __ballot(big); bm; bm &= bm - 1) {   // (wave-uniform)
            const int32_t j = w + (int32_t)(__ffsll((unsigned long long)bm) - 1) * FB_W, oj = o0 + j;
            const int32_t opj = G.perm ? G.perm[oj] : oj;
            const int64_t e0 = ss_off[opj], e1 = ss_off[opj + 1];
            double bb = 0.0;
            for (int64_t e = e0 + lane; e < e1; e += WAVE) {
                const int32_t pp = ss_par[e];
                bb += (double)pw[pp] * sp_cur[pp];
            }
            bb = wave_sum(bb);
            if (lane == 0) lssv[j] = G.alpha * (bb / Ms);
        }
    }
    // the finishing lanes' operands, loaded before the rows so both latencies overlap
    const bool fin = w == 0 && lane < OPB && on;
    const int32_t op = fin && G.perm ? G.perm[o] : o;
    const float uo = fin ? G.u_o[op] : 0.0f;
    const int32_t bidx = (int32_t)blockIdx.x - G.blk0fb;
    const size_t par = (size_t)(px.seq & 1) * (size_t)px.R;   // this round's slots: [par + src] x W words
    if (bidx == 0 && w == 1 && mode) {   // r' maxima riding on the limb sum
        unsigned long long* Mn = G.mslot + (size_t)2 * MSH * ((it % 3 + 1) % 3);
        if (!pxo) {
            if (mode == 1) rmax_put(G, Mn, G.fx_limb + 2 * (size_t)N, lane);
            else rmax_take_bits(G.fx_limb + 2 * (size_t)N, G.nranks, Mn, lane);
        } else if (mode == 1) {   // this rank's maximum into word 2N + rank of its slot on every rank
            const double m = wave_max(bits2d(Mn[MSH + lane]));
            if (lane < px.R)
                __hip_atomic_store((GLB unsigned long long*)px.peers[lane] + px.slots + (par + px.rank) * px.W +
                                       2 * (size_t)N + px.rank,
                                   d2bits(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (pxo && mode == 2) {
        if (px.spin && threadIdx.x == 0) {   // flag (src, bidx) of every source: this round's words are in
            s_ok = 1;
            const unsigned long long need = px.seq + 1, t0 = __builtin_amdgcn_s_memrealtime();
            for (int r = 0; r < px.R && s_ok; ++r)
                while (__hip_atomic_load(preg + px.bflags + (int64_t)r * px.nbf + bidx, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM) < need) {
                    __builtin_amdgcn_s_sleep(2);
                    // a round that already timed out (this call's error word): stop at once instead
                    // of spinning the full timeout again in every later iteration
                    if (__builtin_amdgcn_s_memrealtime() - t0 > px.timeout ||
                        __hip_atomic_load(preg + px.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ull) {
                        s_ok = 0;
                        __hip_atomic_store((GLB unsigned long long*)px.region + px.err, 1ull, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
        } else if (!px.spin && threadIdx.x == 0) {
            s_ok = 1;
        }
        __syncthreads();
        if (!s_ok) return;   // (the error word reports it; the host raises MR_ERR_COMM)
        if (bidx == 0 && w == 1) {   // every rank's r' maximum: word 2N + src of slot src
            unsigned long long b = 0ull;
            for (int j = lane; j < px.R; j += WAVE)
                b = max(b, __hip_atomic_load(preg + px.slots + (par + j) * px.W + 2 * (size_t)N + j, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM));
            const double m = wave_max(bits2d(b));
            if (lane == 0) atomicMax(&G.mslot[(size_t)2 * MSH * ((it % 3 + 1) % 3) + MSH], d2bits(m));
        }
    }
    unsigned long long lo = 0ull, hi = 0ull;
    if (nbl > 0) {
        // the first batch (loaded above), then batches of 16 rows per lane, every load in flight
        // before the sums (indices clamped: the repeats are cache hits and are not added)
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (rfirst + k * stride < nbl) {
                lo += v0[k] & 0xffffffffull;
                hi += v0[k] >> 32;
            }
        for (int32_t r0 = rfirst + 16 * stride; r0 < nbl; r0 += 16 * stride) {
            unsigned long long v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = col[(size_t)min(r0 + k * stride, nbl - 1) * rs];
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (r0 + k * stride < nbl) {
                    lo += v[k] & 0xffffffffull;
                    hi += v[k] >> 32;
                }
        }
    }
    // the wave's row groups of one op meet by lane shuffles, the waves through LDS (integers:
    // order-free)
    for (int m = WAVE / 2; m >= OPB; m >>= 1) {
        lo += (unsigned long long)__shfl_xor((long long)lo, m);
        hi += (unsigned long long)__shfl_xor((long long)hi, m);
    }
    if (lane < OPB) {
        slo[w * WAVE + lane] = lo;
        shi[w * WAVE + lane] = hi;
    }
    __syncthreads();
    if (pxo && mode == 1) {   // push the block's limbs to every rank, then the block's flag there
        if (fin) {
            lo = hi = 0ull;
            for (int k = 0; k < FB_W; ++k) {
                lo += slo[k * WAVE + lane];
                hi += shi[k * WAVE + lane];
            }
            for (int r = 0; r < px.R; ++r) {
                GLB unsigned long long* dst = (GLB unsigned long long*)px.peers[r] + px.slots + (par + px.rank) * px.W;
                __hip_atomic_store(dst + 2 * op, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(dst + 2 * op + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (every wave: the r' word of wave 1 too)
        __syncthreads();
        if ((int32_t)threadIdx.x < px.R && !px.mute) {
            __atomic_thread_fence(__ATOMIC_RELEASE);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store((GLB unsigned long long*)px.peers[threadIdx.x] + px.bflags + (int64_t)px.rank * px.nbf + bidx,
                               (unsigned long long)(px.seq + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (!fin) return;
    lo = hi = 0ull;
    for (int k = 0; k < FB_W; ++k) {
        lo += slo[k * WAVE + lane];
        hi += shi[k * WAVE + lane];
    }
    if (mode == 1) {
        G.fx_limb[2 * op] = lo;
        G.fx_limb[2 * op + 1] = hi;
        return;
    }
    if (mode == 2 && pxo) {   // the R slots in rank order (integers: the all-reduce's sum)
        lo = hi = 0ull;
        for (int r = 0; r < px.R; ++r) {
            const GLB unsigned long long* sl = preg + px.slots + (par + r) * px.W;
            lo += __hip_atomic_load(sl + 2 * op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            hi += __hip_atomic_load(sl + 2 * op + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else if (mode == 2) {
        lo = G.fx_limb[2 * op];
        hi = G.fx_limb[2 * op + 1];
    }
    const int nxt = (it & 1) ^ 1, k3 = it % 3;
    unsigned long long* Mnext = G.mslot + (size_t)2 * MSH * ((k3 + 1) % 3);
    const double ssv = lssv[lane];   // (written before the barrier above)
    // hi, lo < 2^53 (fewer than 2^21 rows over all ranks): both conversions exact, one rounding
    const double sum = ((double)hi * 4294967296.0 + (double)lo) * (o < G.NA ? (G.dscale ? G.dscale[1] : G.fx_iscale) : G.cx_iscale);
    const double v = d * (sum + ssv);      // pagerank.py:122-124
    G.spb[nxt][op] = v;
    const double su = (double)uo * v;
    if (G.su32) {   // (fp32 wide graphs: rounded to float, kept both ways)
        const float f = (float)su;
        G.sub[nxt][o] = (double)f;
        G.suf[nxt][o] = f;
    } else {
        G.sub[nxt][o] = su;   // su in the kernel's labels
    }
    atomicMax(&Mnext[op % MSH], d2bits(v));
}

}  // namespace
