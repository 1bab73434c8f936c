// bevw_gray_stitch.h -- the launchers of the one-channel stitch kernels (bevw_set_channels: a bevw_handle on 8UC1 frames).  Every kernel of
// it has a name of its own (k_stitch_units_gray, k_stitch_tiles_gray, k_stitch_pp_gray: bevw_kernels_gray_stitch.h) and is compiled in
// bevwarp_gray_stitch.hip alone, which defines the functions declared here; the plan's and the main unit's dispatch call them for the
// one-channel steps of a handle.  A launcher queues its kernel on `st`; the caller reads hipGetLastError() as after its own launches.
#pragma once
#include "bevw_planapi.h"

namespace bevw {

struct PlanArgs;   // bevw_plan.h

// the unit kernel of a step (plan_gray_stitch_step): grid and unit list as for the other formats, a.un_gsrc = Plan::units[kLayoutGray];
// a.car has rows of car_pitch bytes
void gray_stitch_launch_units(const PlanArgs &a, int car_pitch, bool blend, hipStream_t st);
// the per-tap tile kernel of a step (plan_gray_stitch_step): the base tiles no unit owns
void gray_stitch_launch_tiles(const PlanArgs &a, int car_pitch, bool blend, hipStream_t st);
// the per-pixel stitch of one batch chunk (run_device): `frames` holds sets of four fw x fh planes, `car` is dense or nullptr, `out` has rows
// of `pitch` bytes
void gray_stitch_launch_pp(hipStream_t st, dim3 grid, bool blend, const uint8_t *frames, int fw, int fh, const StitchTables &T, int bw, int bh,
                           const uint8_t *car, uint8_t *out, int pitch, int ties_even);

}  // namespace bevw
