// bevw_nearest.h -- the launchers of the nearest-neighbour kernels of a one-channel remapper (bevw_remapper_set_interpolation:
// cv2.INTER_NEAREST on 8UC1 and 16UC1 sources).  Every such kernel has a name of its own (k_units_nn8 / nn16, k_tiles_nn8 / nn16,
// k_remap_nn8 / nn16) and is compiled in bevwarp_nearest.hip alone, which defines the functions declared here; the plan's and the main
// unit's dispatch call them for nearest steps.  A launcher queues its kernel on `st`; the caller reads hipGetLastError() as after its own
// launches.  deep: 16 bits per texel.
#pragma once
#include "bevw_planapi.h"

namespace bevw {

struct PlanArgs;   // bevw_plan.h

// the unit kernel of a step (plan_gray_step): grid and unit list as for linear steps, a.un_gsrc = Plan::units[kLayoutGray] (the 16-bit
// kernel doubles the offsets), a.set_stride = the bytes of a frame set
void nearest_launch_units(const PlanArgs &a, hipStream_t st, bool deep);
// the per-tap tile kernel of a step (plan_gray_step): the base tiles no unit owns
void nearest_launch_tiles(const PlanArgs &a, hipStream_t st, bool deep);
// the per-pixel kernel of one batch chunk (remap_launch): `src` and `dst` hold one uint8 (deep: one little-endian uint16) per pixel
void nearest_launch_remap(hipStream_t st, dim3 grid, bool deep, const void *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw, int dh,
                          void *dst);

}  // namespace bevw
