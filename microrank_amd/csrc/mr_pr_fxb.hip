// k_fx_b's unit: the kernel (mr_pr_fxb_dev.h) is instantiated here and nowhere else, for the two block
// sizes, and leaves as a host function pointer for iterate (mr_pagerank.hip), which launches it.
#include "mr_pr_fxb_dev.h"
#include "mr_pr_iter.h"

FxB fx_b_kernel(bool small) { return small ? k_fx_b<FB_W_SMALL> : k_fx_b<FB_W>; }
