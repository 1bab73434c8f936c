// bevwarp_yuv422.hip -- the packed 4:2:2 input formats of libbevwarp.so (bevw_set_input_format: YUYV, UYVY): the one translation unit that
// instantiates the kernels that read such frames (bevw_kernels_yuv422.h): the unit kernel, the per-tap tile kernel, the balance scratch
// and the per-pixel, remap and V-sum kernels.  Their bodies are the shared device functions and kernel bodies of the other formats'
// kernels with a 4:2:2 source; this unit compiles no kernel of another unit.  It defines the launchers of bevw_yuv422.h.
#define BEVW_PLAN_SHARED_ONLY 1   // bevw_plan.h without the plan's own kernels and host code
#include "bevw_plan.h"
#include "bevw_kernels_yuv422.h"

namespace bevw {

void yuv422_launch_units(const PlanArgs &a, hipStream_t st, bool blend, bool out_nv12)
{
    const dim3 grid(plan_grid(a)), block(kUnitThreads);
    with_flags([&](auto bl, auto on) {
        if constexpr (on) hipLaunchKernelGGL((k_units_out_yuv422<bl>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_units_yuv422<bl>), grid, block, 0, st, a);
    }, blend, out_nv12);
}

void yuv422_launch_stitch_plan(const PlanArgs &a, hipStream_t st, bool blend, bool lum, bool sums, bool out_nv12)
{
    const dim3 grid(plan_grid(a)), block(256);
    // (as for the other formats: NV12 images exist without the luminance round trip and channel sums only)
    if (out_nv12) with_flags([&](auto bl) { hipLaunchKernelGGL((k_stitch_plan_yuv422<bl, false, false, true>), grid, block, 0, st, a); }, blend);
    else with_flags([&](auto bl, auto lm, auto sm) { hipLaunchKernelGGL((k_stitch_plan_yuv422<bl, lm, sm, false>), grid, block, 0, st, a); }, blend, lum, sums);
}

void yuv422_launch_lum_groups(hipStream_t st, dim3 grid, const uint8_t *frames, uint8_t *scratch, size_t set_bytes, size_t scratch_stride, uint32_t frame_bytes,
                              const uint32_t *groups, int ngroups, const int *deltas, const HsvTables *tab, uint32_t blocks_per_frame, uint32_t nframes,
                              Yuv422Order order)
{
    hipLaunchKernelGGL(k_lum_groups_yuv422, grid, dim3(256), 0, st, frames, scratch, set_bytes, scratch_stride, frame_bytes, groups, ngroups, deltas, tab,
                       blocks_per_frame, nframes, order);
}

void yuv422_launch_stitch_pp(hipStream_t st, dim3 grid, bool blend, bool balance, bool out_nv12, const uint8_t *frames, int fw, int fh, const StitchTables &T,
                             int bw, int bh, const int *deltas, const HsvTables *tab, const uint8_t *car, unsigned long long *chsums, uint8_t *out,
                             int ties_even, Yuv422Order order)
{
    const uint32_t ypos = order.ysel & 1u;
    auto launch = [&](auto bl, auto ba, auto on) {
        hipLaunchKernelGGL((k_stitch_pp_yuv422<bl, ba, on>), grid, dim3(256), 0, st, frames, fw, fh, T, bw, bh, deltas, tab, car, chsums, out, ties_even, ypos);
    };
    if (out_nv12) with_flags([&](auto bl) { launch(bl, std::false_type{}, std::true_type{}); }, blend);
    else with_flags([&](auto bl, auto ba) { launch(bl, ba, std::false_type{}); }, blend, balance);
}

void yuv422_launch_remap_lut(hipStream_t st, dim3 grid, bool out_nv12, const uint8_t *src, int sw, int sh, const int16_t *map1, const uint16_t *map2, int dw,
                             int dh, uint8_t *dst, int ties_even, Yuv422Order order)
{
    with_flags([&](auto on) {
        hipLaunchKernelGGL((k_remap_lut_yuv422<on>), grid, dim3(256), 0, st, src, sw, sh, map1, map2, dw, dh, dst, ties_even, order.ysel & 1u);
    }, out_nv12);
}

void yuv422_launch_vsum(hipStream_t st, dim3 grid, const uint8_t *frames, size_t frame_bytes, int vec_ok, unsigned long long *sums, int part_stride,
                        Yuv422Order order)
{
    hipLaunchKernelGGL(k_vsum_yuv422, grid, dim3(256), 0, st, frames, frame_bytes, vec_ok, sums, part_stride, order);
}

}  // namespace bevw
