// bevw_gray.h -- the launchers of the one-channel kernels (bevw_remapper_set_channels: 8UC1 sources and destinations of a remapper).  Every
// kernel that reads such frames has a name of its own (k_units_gray, k_stitch_plan_gray, k_remap_lut_gray) and is compiled in
// bevwarp_gray.hip alone, which defines the functions declared here; the plan's and the main unit's dispatch call them for one-channel
// steps.  A launcher queues its kernel on `st`; the caller reads hipGetLastError() as after its own launches.
#pragma once
#include "bevw_planapi.h"

namespace bevw {

struct PlanArgs;   // bevw_plan.h

// the unit kernel of a step (plan_gray_step): grid and unit list as for the other formats, a.un_gsrc = Plan::units[kLayoutGray]
void gray_launch_units(const PlanArgs &a, hipStream_t st);
// the per-tap tile kernel of a step (plan_gray_step): the base tiles no unit owns
void gray_launch_stitch_plan(const PlanArgs &a, hipStream_t st);
// k_remap_lut of one batch chunk (remap_launch): `src` and `dst` hold one byte per pixel
void gray_launch_remap_lut(hipStream_t st, dim3 grid, const uint8_t *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw, int dh,
                           uint8_t *dst, int ties_even);

}  // namespace bevw
