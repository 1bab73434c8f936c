// bevwarp_gray.hip -- the one-channel mode of libbevwarp.so's remappers (bevw_remapper_set_channels: 8UC1 sources and destinations): the
// one translation unit that instantiates the kernels that read such frames (bevw_kernels_gray.h): the unit kernel, the per-tap tile kernel
// and the per-pixel kernel.  They run the plan, the unit partition and the entries of the three-channel remapper on one byte per texel;
// this unit compiles no kernel of another unit.  It defines the launchers of bevw_gray.h.
#define BEVW_PLAN_SHARED_ONLY 1   // bevw_plan.h without the plan's own kernels and host code
#include "bevw_plan.h"
#include "bevw_kernels_gray.h"

namespace bevw {

void gray_launch_units(const PlanArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_units_gray, dim3(plan_grid(a)), dim3(kUnitThreads), 0, st, a);
}

void gray_launch_stitch_plan(const PlanArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_stitch_plan_gray, dim3(plan_grid(a)), dim3(256), 0, st, a);
}

void gray_launch_remap_lut(hipStream_t st, dim3 grid, const uint8_t *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw, int dh,
                           uint8_t *dst, int ties_even)
{
    hipLaunchKernelGGL(k_remap_lut_gray, grid, dim3(256), 0, st, src, sw, sh, map1, map2, dw, dh, dst, ties_even);
}

}  // namespace bevw
