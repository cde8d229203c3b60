// hmk_grid.h -- the workgroup count of a grid-stride launch, as the launchers of k_linkage, k_split, k_pairs, k_assign, k_match,
// k_merge, k_search, k_components, k_align, k_survey, k_separation, k_sweep, k_representatives, k_density, k_profile, k_scan, k_orders and k_traceback.hip ask for it.  Their kernels let a workgroup take a second chunk, tile or run once the input
// outgrows the grid (65,536 chunks, 1,024 long runs, ...), which no test input does: the test switch HMK_TEST_GRID_CAP=n (Switches::read,
// hmk_common.cpp) gives every such launch min(its own grid, n) workgroups instead, so that the work loops
// run their later iterations at test sizes (tests/test_work_loops.py).  Host code only: no kernel knows of it.
#ifndef HMK_GRID_H
#define HMK_GRID_H

#include <stdint.h>

namespace hmk {

void set_test_grid_cap(int cap);   // below 1: no cap (the default)
// min(wanted, cap); a launch the cap cuts writes "[hmk grid] <kernel> <wanted> -> <launched>" to stderr
uint32_t capped_grid(const char *kernel, uint32_t wanted);

}  // namespace hmk
#endif
