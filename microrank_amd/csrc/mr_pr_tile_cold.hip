// The unit of the iteration's other kernels, each instantiated here and nowhere else: the tile path
// of general graphs (k_iter_a, k_iter_b: mr_pr_tile_dev.h) and the wide graphs' cold halves
// (k_cold_trace, k_cold_ops: mr_pr_cold_dev.h).  They leave as host function pointers for iterate
// (mr_pagerank.hip), which launches them.
#include "mr_pr_cold_dev.h"
#include "mr_pr_iter.h"
#include "mr_pr_tile_dev.h"

IterA iter_a_kernel(bool fp32) { return fp32 ? k_iter_a<float> : k_iter_a<double>; }
IterB iter_b_kernel() { return k_iter_b; }
ColdTrace cold_trace_kernel() { return k_cold_trace; }
ColdOps cold_ops_kernel(bool fp32) { return fp32 ? k_cold_ops<float> : k_cold_ops<double>; }
