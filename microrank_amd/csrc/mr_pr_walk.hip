// The walk's unit: k_tr_a (mr_pr_walk_dev.h) is instantiated here and nowhere else -- once per entry of
// the list below -- and leaves as a host function pointer: tr_kernel, called by finalise_launch
// (mr_pr_launch.hip) for the launch and by plan_resident (mr_pr_plan.hip) for its occupancy.
#include <type_traits>

#include "mr_pr_iter.h"
#include "mr_pr_walk_dev.h"

namespace {

struct TrVariant {
    bool fp32;
    int mode, NT, ext;
    TrA k;
};
#define TR_V(Q, M, NT, X) {std::is_same<Q, float>::value, M, NT, X, k_tr_a<Q, M, NT, X>}
#define TR_V4(M, X) TR_V(double, M, 512, X), TR_V(double, M, 1024, X), TR_V(float, M, 512, X), TR_V(float, M, 1024, X)
// Every k_tr_a that is built: 12 + 16 + 2 = 30.  Only WV_SU_ALL has the short-tile walk, the one
// place EXT is read (tr_walk_short; the 1024-thread ones also carry the hot ops).  RUNS is never
// beside KINDS or COLD, W32 only with COLD alone and only on floats (TrSu).
const TrVariant TR_BUILT[] = {
    // every su mode, both block sizes, both precisions
    TR_V4(WV_SU_GLOBAL, 0), TR_V4(WV_SU_ALL, 0), TR_V4(WV_SU_HOT, 0),
    // su in LDS: kind multiplicities, a cold side, both, merged runs
    TR_V4(WV_SU_ALL, TR_X_KINDS), TR_V4(WV_SU_ALL, TR_X_COLD), TR_V4(WV_SU_ALL, TR_X_KINDS | TR_X_COLD),
    TR_V4(WV_SU_ALL, TR_X_RUNS),
    // fp32 wide graphs: float su and warm labels in LDS
    TR_V(float, WV_SU_ALL, 512, TR_X_COLD | TR_X_W32), TR_V(float, WV_SU_ALL, 1024, TR_X_COLD | TR_X_W32)};
#undef TR_V4
#undef TR_V

}  // namespace

// A launch is one variant for all its graphs.  Merged runs beside kind multiplicities or a cold
// side: no such variant is built, so the runs are dropped (every lane walks its own trace -- the
// same sums).  A cold side alone on a plan with float su (FxPlan::w32): the W32 walk.
int tr_launch_ext(int any, bool w32) {
    if ((any & TR_X_RUNS) && (any & (TR_X_KINDS | TR_X_COLD))) any &= ~TR_X_RUNS;
    if (any == TR_X_COLD && w32) any |= TR_X_W32;
    return any;
}

// (the modes without a short-tile walk never read EXT: their one variant serves every launch)
TrA tr_kernel(bool fp32, int mode, int NT, int ext) {
    if (mode != WV_SU_ALL) ext = 0;
    for (const TrVariant& v : TR_BUILT)
        if (v.fp32 == fp32 && v.mode == mode && v.NT == NT && v.ext == ext) return v.k;
    return nullptr;
}
