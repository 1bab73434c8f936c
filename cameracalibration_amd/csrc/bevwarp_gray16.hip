// bevwarp_gray16.hip -- the 16-bit one-channel mode of libbevwarp.so's remappers (bevw_remapper_set_depth: 16UC1 sources and destinations):
// the one translation unit that instantiates the kernels that read such frames (bevw_kernels_gray16.h): the unit kernel, the per-tap tile
// kernel and the per-pixel kernel.  They run the plan, the unit partition, the entries and the group list of the 8-bit one-channel remapper
// on two bytes per texel with cv2.remap's float arithmetic for CV_16U; this unit compiles no kernel of another unit.  It defines the
// launchers of bevw_gray16.h.
#define BEVW_PLAN_SHARED_ONLY 1   // bevw_plan.h without the plan's own kernels and host code
#include "bevw_plan.h"
#include "bevw_kernels_gray16.h"
#include "bevw_gray16.h"

namespace bevw {

void gray16_launch_units(const PlanArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_units_gray16, dim3(plan_grid(a)), dim3(kUnitThreads), 0, st, a);
}

void gray16_launch_stitch_plan(const PlanArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_stitch_plan_gray16, dim3(plan_grid(a)), dim3(256), 0, st, a);
}

void gray16_launch_remap_lut(hipStream_t st, dim3 grid, const uint16_t *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw, int dh,
                             uint16_t *dst)
{
    hipLaunchKernelGGL(k_remap_lut_gray16, grid, dim3(256), 0, st, src, sw, sh, map1, map2, dw, dh, dst);
}

}  // namespace bevw
