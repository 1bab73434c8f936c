// bevw_gray16.h -- the launchers of the 16-bit one-channel kernels (bevw_remapper_set_depth: 16UC1 sources and destinations of a remapper).
// Every kernel that reads such frames has a name of its own (k_units_gray16, k_stitch_plan_gray16, k_remap_lut_gray16) and is compiled in
// bevwarp_gray16.hip alone, which defines the functions declared here; the plan's and the main unit's dispatch call them for 16-bit steps.
// A launcher queues its kernel on `st`; the caller reads hipGetLastError() as after its own launches.
#pragma once
#include "bevw_planapi.h"

namespace bevw {

struct PlanArgs;   // bevw_plan.h

// the unit kernel of a step (plan_gray16_step): grid and unit list as for 8 bits, a.un_gsrc = Plan::units[kLayoutGray] (the kernel doubles
// the offsets), a.set_stride = the bytes of a frame set
void gray16_launch_units(const PlanArgs &a, hipStream_t st);
// the per-tap tile kernel of a step (plan_gray16_step): the base tiles no unit owns
void gray16_launch_stitch_plan(const PlanArgs &a, hipStream_t st);
// k_remap_lut of one batch chunk (remap_launch): `src` and `dst` hold one little-endian uint16 per pixel
void gray16_launch_remap_lut(hipStream_t st, dim3 grid, const uint16_t *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw, int dh,
                             uint16_t *dst);

}  // namespace bevw
