// What the launch plan (mr_pr_plan.hip), the launch description (mr_pr_launch.hip) and the walk kernel
// (k_tr_a, mr_pr_walk_dev.h) must agree on, so host and device both include it: the LDS budget, the su
// modes, the bits of k_tr_a's variant and the kernel's LDS image.
#pragma once
#include <algorithm>

#include "mr_pr_internal.h"

// ---------------------------------------------------------------- LDS budget and su modes
constexpr size_t WV_LDS_MAX = 160 * 1024 - 512;
// su modes of k_tr_a: global gathers only / every op's su in LDS / the n_hot most covered ops' su in
// LDS (relabelled graphs, ops [0, n_hot)), the rest gathered
enum { WV_SU_GLOBAL = 0, WV_SU_ALL = 1, WV_SU_HOT = 2 };

// ---------------------------------------------------------------- k_tr_a's variant (its EXT parameter)
// A set of bits: what some fused graph of the launch carries, and so what the short-tile walk of the
// su-in-LDS mode (WV_SU_ALL) compiles in.  The other modes have no short-tile walk and build EXT 0
// only.  Built: 0, KINDS, COLD, KINDS | COLD, RUNS, COLD | W32 (the list: mr_pr_walk.hip, TR_BUILT;
// the rule from a launch's graphs to one of them: tr_launch_ext).
constexpr int TR_X_KINDS = 1;   // kind multiplicities (GDev::mw_tp: kind-compressed graphs)
constexpr int TR_X_COLD = 2;    // a cold side (GDev::cold_acc: wide graphs)
constexpr int TR_X_RUNS = 4;    // merged runs of identical traces (GDev::trun: layout-order window graphs)
constexpr int TR_X_W32 = 8;     // with COLD, fp32 only: su as floats, the warm cold labels' su in LDS

// ---------------------------------------------------------------- k_tr_a's LDS image
struct TrLds {
    size_t su, lacc, hs, sp, total;
    bool su_lds;      // every op's su fits beside the accumulator (interleaved: 16 B per op)
    bool hot_ok;      // WV_SU_ALL: the hot-op mask sums (256 doubles) fit too
    int32_t n_hot;    // WV_SU_HOT: su of ops [0, n_hot) in LDS
    // the accumulator first, then su (8-B strides: a 32-lane read group spreads over 32 bank
    // pairs, a 16-lane atomic group over 16)
    // pf (every op's su in LDS only): s itself beside su (the launch finished the previous iteration)
    // w32 (fp32 wide graphs, k_tr_a EXT & TR_X_W32): su as 4-B floats -- the hot ops, their 64 pad slots,
    // then n_warm "warm" cold labels (NA + j at slot NA + 64 + j) in the space the floats free
    int32_t n_warm;
    __host__ __device__ TrLds(int32_t N, int mode, bool pf = false, bool w32 = false) {
        const size_t ns = (size_t)N + TR_PAD;
        su_lds = ns * 16 <= WV_LDS_MAX;
        const bool all = mode == WV_SU_ALL && su_lds;
        const size_t accb = (ns * 8 + 15) / 16 * 16;
        n_hot = 0;
        n_warm = 0;
        if (mode == WV_SU_HOT && accb < WV_LDS_MAX)
            n_hot = (int32_t)std::min<size_t>((size_t)N, (WV_LDS_MAX - accb) / 8 / 64 * 64);
        lacc = 0;
        su = accb;
        total = all ? 2 * accb : accb + (size_t)n_hot * 8;
        if (all && w32 && !pf) {   // (the hot-op mask sums keep their 2 KB)
            const size_t fl = (WV_LDS_MAX - accb - 256 * 8 - 16) / 4;
            n_warm = fl > ns ? (int32_t)((fl - ns) / 64 * 64) : 0;
            total = accb + ((ns + (size_t)n_warm) * 4 + 15) / 16 * 16;
        }
        sp = total;
        if (pf && all) total += accb;
        hs = total;
        hot_ok = all && total + 256 * 8 <= WV_LDS_MAX;
        if (hot_ok) total += 256 * 8;
    }
};
