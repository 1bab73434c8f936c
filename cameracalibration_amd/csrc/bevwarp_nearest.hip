// bevwarp_nearest.hip -- the nearest-neighbour mode of libbevwarp.so's one-channel remappers (bevw_remapper_set_interpolation:
// cv2.INTER_NEAREST on class-ID maps, instance-ID maps and masks): the one translation unit that instantiates the kernels of that mode
// (bevw_kernels_nearest.h) -- the unit kernel, the per-tap tile kernel and the per-pixel kernel, each at 8 and at 16 bits.  They run the
// plan, the unit partition, the entries and the group list of the linear one-channel remapper with a lane body that picks one texel; this
// unit compiles no kernel of another unit.  It defines the launchers of bevw_nearest.h.
#define BEVW_PLAN_SHARED_ONLY 1   // bevw_plan.h without the plan's own kernels and host code
#define BEVW_GRAY_SHARED_ONLY 1   // bevw_kernels_gray.h without its kernels
#include "bevw_plan.h"
#include "bevw_kernels_gray.h"
#include "bevw_kernels_nearest.h"
#include "bevw_nearest.h"

namespace bevw {

void nearest_launch_units(const PlanArgs &a, hipStream_t st, bool deep)
{
    if (deep) hipLaunchKernelGGL(k_units_nn16, dim3(plan_grid(a)), dim3(kUnitThreads), 0, st, a);
    else hipLaunchKernelGGL(k_units_nn8, dim3(plan_grid(a)), dim3(kUnitThreads), 0, st, a);
}

void nearest_launch_tiles(const PlanArgs &a, hipStream_t st, bool deep)
{
    if (deep) hipLaunchKernelGGL(k_tiles_nn16, dim3(plan_grid(a)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_tiles_nn8, dim3(plan_grid(a)), dim3(256), 0, st, a);
}

void nearest_launch_remap(hipStream_t st, dim3 grid, bool deep, const void *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw, int dh,
                          void *dst)
{
    if (deep)
        hipLaunchKernelGGL(k_remap_nn16, grid, dim3(256), 0, st, static_cast<const uint16_t *>(src), sw, sh, map1, map2, dw, dh, static_cast<uint16_t *>(dst));
    else
        hipLaunchKernelGGL(k_remap_nn8, grid, dim3(256), 0, st, static_cast<const uint8_t *>(src), sw, sh, map1, map2, dw, dh, static_cast<uint8_t *>(dst));
}

}  // namespace bevw
