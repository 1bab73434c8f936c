// bevw_yuv422.h -- the launchers of the packed 4:2:2 kernels (bevw_set_input_format: YUYV, UYVY).  Every kernel that reads such frames has a
// name of its own (k_units_yuv422, k_units_out_yuv422, k_stitch_plan_yuv422, k_stitch_pp_yuv422, k_remap_lut_yuv422, k_vsum_yuv422,
// k_lum_groups_yuv422) and is compiled in bevwarp_yuv422.hip alone, which defines the functions declared here; the plan's and the main
// unit's dispatch call them for 4:2:2 steps.  A launcher queues its kernel on `st`; the caller reads hipGetLastError() as after its own launches.
#pragma once
#include "bevw_planapi.h"

namespace bevw {

struct PlanArgs;   // bevw_plan.h

// the unit kernel of a step (plan_launch_units): grid and tile list as for the other formats, a.un_gsrc = Plan::units[kLayoutYuv422]
void yuv422_launch_units(const PlanArgs &a, hipStream_t st, bool blend, bool out_nv12);
// the per-tap tile kernel of a step (plan_stitch_impl); OUT_NV12 exists without the luminance round trip and channel sums only
void yuv422_launch_stitch_plan(const PlanArgs &a, hipStream_t st, bool blend, bool lum, bool sums, bool out_nv12);
// k_lum_groups of one batch chunk (plan_lum_band)
void yuv422_launch_lum_groups(hipStream_t st, dim3 grid, const uint8_t *frames, uint8_t *scratch, size_t set_bytes, size_t scratch_stride, uint32_t frame_bytes,
                              const uint32_t *groups, int ngroups, const int *deltas, const HsvTables *tab, uint32_t blocks_per_frame, uint32_t nframes,
                              Yuv422Order order);
// k_stitch_pp of one batch chunk (stitch_per_pixel); OUT_NV12 exists without balance only
void yuv422_launch_stitch_pp(hipStream_t st, dim3 grid, bool blend, bool balance, bool out_nv12, const uint8_t *frames, int fw, int fh, const StitchTables &T,
                             int bw, int bh, const int *deltas, const HsvTables *tab, const uint8_t *car, unsigned long long *chsums, uint8_t *out,
                             int ties_even, Yuv422Order order);
// k_remap_lut of one batch chunk (remap_launch)
void yuv422_launch_remap_lut(hipStream_t st, dim3 grid, bool out_nv12, const uint8_t *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw,
                             int dh, uint8_t *dst, int ties_even, Yuv422Order order);
// k_vsum of one chunk of frames (vsum_launch)
void yuv422_launch_vsum(hipStream_t st, dim3 grid, const uint8_t *frames, size_t frame_bytes, int vec_ok, unsigned long long *sums, int part_stride,
                        Yuv422Order order);

}  // namespace bevw
