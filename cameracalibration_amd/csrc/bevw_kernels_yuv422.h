// bevw_kernels_yuv422.h -- every kernel that reads packed 4:2:2 camera frames (bevw_set_input_format: YUYV, UYVY), under names of their own.
// Included by bevwarp_yuv422.hip alone, behind bevw_plan.h with BEVW_PLAN_SHARED_ONLY: the kernels are the shared device functions
// (plan_unit_any, eval_entry, remap_u8c3_px) and the shared kernel bodies (bevw_body_*.h) of the other formats' kernels with a 4:2:2
// source.  The byte order is a kernel argument (Yuv422Order, or bit 0 of its Y selector), so the two orders run the same kernels.
#pragma once
#include "bevw_plan.h"

namespace bevw {

// ---- the unit kernel (bevw_unit.h) --------------------------------------------------------------------------------------------------
// Packed 4:2:2 frame sets (bevw_set_input_format: YUYV, UYVY): the same launch over the kLayoutYuv422 instantiation of plan_unit_run, writing BGR
// (k_units_yuv422) or NV12 images (k_units_out_yuv422); the byte order rides in a.yuv422.
template <bool BLEND>
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_units_yuv422(PlanArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[kUnitMaxGroups * 32];
    plan_unit_any<BLEND, false, kLayoutYuv422, false>(a, blockIdx.x, patch, nullptr);
}
template <bool BLEND>
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_units_out_yuv422(PlanArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[kUnitMaxGroups * 32];
    plan_unit_any<BLEND, false, kLayoutYuv422, true>(a, blockIdx.x, patch, nullptr);
}

// ---- the per-tap tile kernel and the balance scratch (bevw_plan.h) ------------------------------------------------------------------------
// k_stitch_plan on packed 4:2:2 frame sets (a.yuv422)
template <bool BLEND, bool LUM, bool SUMS, bool OUT_NV12>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) k_stitch_plan_yuv422(PlanArgs a)
{
    constexpr SrcLayout SRC = kLayoutYuv422;
#include "bevw_body_stitch_plan.h"
}

// k_lum_groups on packed 4:2:2 frame sets: `groups` holds one offset per group (unit_gsrc_yuv422)
static __global__ void __launch_bounds__(256) k_lum_groups_yuv422(const uint8_t *__restrict__ frames, uint8_t *__restrict__ scratch, size_t set_bytes,
                                                                   size_t scratch_stride, uint32_t frame_bytes, const uint32_t *__restrict__ groups, int ngroups,
                                                                   const int *__restrict__ deltas, const HsvTables *__restrict__ tab,
                                                                   uint32_t blocks_per_frame, uint32_t nframes, Yuv422Order order)
{
    constexpr SrcLayout SRC = kLayoutYuv422;
    const Nv12Surface *const surf = nullptr;
#include "bevw_body_lum_groups.h"
}

// ---- the per-pixel, remap and V-sum kernels (bevw_kernels.h) ---------------------------------------------------------------------------
// k_stitch_pp on packed 4:2:2 frame sets
template <bool BLEND, bool BAL, bool OUT_NV12>
static __global__ void k_stitch_pp_yuv422(const uint8_t *__restrict__ frames, int fw, int fh, StitchTables T, int bw, int bh,
                                          const int *__restrict__ deltas, const HsvTables *__restrict__ tab,
                                          const uint8_t *__restrict__ car, unsigned long long *__restrict__ chsums,
                                          uint8_t *__restrict__ out, int ties_even, uint32_t ypos)
{
    constexpr SrcLayout SRC = kLayoutYuv422;
    const Nv12Surface *const surf = nullptr;
    constexpr int src_pitch = 0;
#include "bevw_body_stitch_pp.h"
}

// k_remap_lut on packed 4:2:2 sources
template <bool OUT_NV12>
static __global__ void k_remap_lut_yuv422(const uint8_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                          const uint16_t *__restrict__ map2, int dw, int dh, uint8_t *__restrict__ dst, int ties_even, uint32_t ypos)
{
    constexpr SrcLayout SRC = kLayoutYuv422;
    const Nv12Surface *const surf = nullptr;
    constexpr int src_pitch = 0;
#include "bevw_body_remap_lut.h"
}

// k_vsum over packed 4:2:2 frames (YUYV / UYVY; frame_bytes = fw * fh * 2, fw even): a frame is a flat run of 4-byte texel pairs, and V is
// summed over every converted texel.  vec_ok (16-byte aligned frames): 16-byte streaming loads of 8 texels, the tail in 4-byte pairs; else
// byte loads.  The sums leave as k_vsum's do (part_stride).
typedef uint32_t vsum_u32x4 __attribute__((ext_vector_type(4)));
static __global__ void k_vsum_yuv422(const uint8_t *__restrict__ frames, size_t frame_bytes, int vec_ok, unsigned long long *__restrict__ sums,
                                     int part_stride, Yuv422Order order)
{
    const uint8_t *f = frames + (size_t)blockIdx.y * frame_bytes;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
    auto v = [](uint32_t t) { return max(t & 255u, max((t >> 8) & 255u, t >> 16)); };
    auto quad = [&](uint32_t lo, uint32_t hi) {   // texels x .. x+3
        uint32_t y, uv, P[4];
        yuv422_split(lo, hi, order, y, uv);
        nv12_row_bgr<4>(y, uv, P);
        return v(P[0]) + v(P[1]) + v(P[2]) + v(P[3]);
    };
    unsigned acc = 0;
    const size_t npieces = vec_ok ? frame_bytes / 16 : 0;
    const vsum_u32x4 *fp = reinterpret_cast<const vsum_u32x4 *>(f);
    for (size_t i = tid; i < npieces; i += nthreads) {
        const vsum_u32x4 w = once_load<BEVW_VSUM_NT>(fp + i);   // (bevw_device.h: the frames pass once)
        acc += quad(w.x, w.y) + quad(w.z, w.w);
    }
    // the texel pairs whole pieces do not cover
    const uint32_t ypos = order.ysel & 1u;
    for (size_t t = npieces * 4 + tid; t * 4 + 3 < frame_bytes; t += nthreads) {
        const uint8_t *p = f + t * 4;
        const Nv12Chroma c = nv12_chroma(p[1 - ypos], p[3 - ypos]);
        acc += v(nv12_bgr(p[ypos], c)) + v(nv12_bgr(p[2 + ypos], c));
    }
    __shared__ unsigned long long part[16];
    unsigned long long s = wave_sum_u64(acc);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) part[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int i2 = 0; i2 < (int)(blockDim.x >> 6); ++i2) t += part[i2];
        if (part_stride > 0) sums[(size_t)blockIdx.y * part_stride + blockIdx.x] = t;
        else atomicAdd(&sums[blockIdx.y], t);
    }
}

}  // namespace bevw
