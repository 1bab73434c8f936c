// bevwarp_gray_stitch.hip -- the one-channel mode of libbevwarp.so's handles (bevw_set_channels: the four-camera stitch on 8UC1 frames): the
// one translation unit that instantiates the kernels of bevw_kernels_gray_stitch.h -- the unit kernel over every class of the partition,
// the per-tap tile kernel and the per-pixel stitch, each direct and blend.  It compiles no kernel of another unit (the one-channel
// remapper's stay in bevwarp_gray.hip).  It defines the launchers of bevw_gray_stitch.h.
#define BEVW_PLAN_SHARED_ONLY 1   // bevw_plan.h without the plan's own kernels and host code
#define BEVW_GRAY_SHARED_ONLY 1   // bevw_kernels_gray.h without its kernels
#include "bevw_plan.h"
#include "bevw_kernels_gray_stitch.h"

namespace bevw {

void gray_stitch_launch_units(const PlanArgs &a, int car_pitch, bool blend, hipStream_t st)
{
    const GrayStitchArgs g = {a, car_pitch};
    if (blend) hipLaunchKernelGGL((k_stitch_units_gray<true>), dim3(plan_grid(a)), dim3(kUnitThreads), 0, st, g);
    else hipLaunchKernelGGL((k_stitch_units_gray<false>), dim3(plan_grid(a)), dim3(kUnitThreads), 0, st, g);
}

void gray_stitch_launch_tiles(const PlanArgs &a, int car_pitch, bool blend, hipStream_t st)
{
    const GrayStitchArgs g = {a, car_pitch};
    if (blend) hipLaunchKernelGGL((k_stitch_tiles_gray<true>), dim3(plan_grid(a)), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_stitch_tiles_gray<false>), dim3(plan_grid(a)), dim3(256), 0, st, g);
}

void gray_stitch_launch_pp(hipStream_t st, dim3 grid, bool blend, const uint8_t *frames, int fw, int fh, const StitchTables &T, int bw, int bh,
                           const uint8_t *car, uint8_t *out, int pitch, int ties_even)
{
    if (blend) hipLaunchKernelGGL((k_stitch_pp_gray<true>), grid, dim3(256), 0, st, frames, fw, fh, T, bw, bh, car, out, pitch, ties_even);
    else hipLaunchKernelGGL((k_stitch_pp_gray<false>), grid, dim3(256), 0, st, frames, fw, fh, T, bw, bh, car, out, pitch, ties_even);
}

}  // namespace bevw
