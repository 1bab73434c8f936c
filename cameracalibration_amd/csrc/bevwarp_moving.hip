// bevwarp_moving.hip -- the stitch with a homography per frame set of libbevwarp.so's handles (bevw_run_homographies_device: moving
// extrinsics): the one translation unit that instantiates k_stitch_moving (bevw_kernels_moving.h), direct and blend.  It compiles no kernel
// of another unit.  It defines the launcher of bevw_moving.h.
#include "bevw_kernels_moving.h"

namespace bevw {

void moving_launch_stitch(hipStream_t st, const MovingArgs &a, bool blend)
{
    const dim3 grid((a.bw + kMovingTileW - 1) / kMovingTileW, (a.bh + kMovingTileH - 1) / kMovingTileH, (a.batch + a.nb - 1) / a.nb);
    if (blend) hipLaunchKernelGGL((k_stitch_moving<true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_stitch_moving<false>), grid, dim3(256), 0, st, a);
}

}  // namespace bevw
