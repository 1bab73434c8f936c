// bevw_kernels_moving.h -- the kernel of the stitch with a homography per frame set (bevw_run_homographies_device), under a name of its own.
// Included by bevwarp_moving.hip alone.
//
// A handle's BEV tables are cv2.warpPerspective(undistort maps, H) (Camera.get_bev_maps; k_bev_lut) and its stitch is cv2.remap(frame, BEV
// tables) per camera (k_stitch_pp).  Both are functions of one destination pixel, so a step whose H changes per frame set fuses them: per
// pixel, frame set and contributing camera
//   1. perspective_coord in fp64 with the frame set's inverse homography (the host's invert3x3), the column blocks of warpPerspective;
//   2. the four taps of und1 (int16 x 2) and of und2 (uint16) with float weights (remap_f32_px; und2 through warp_f32_px where the handle's
//      BEVW_COMPAT_WARP selects a float32 member), cvRound, saturate_cast to int16 / uint16: the table entry k_bev_lut would have stored;
//   3. the four taps of the frame (remap_u8c3_px, the handle's tie rule);
//   4. the mask (direct) or the blend weight, saturating adds in camera order, then the car.
// Every function named is the one the static kernels call (bevw_device.h), so the bytes are those of a handle rebuilt with that H.  A BEV
// pixel whose position falls outside the undistorted grid reads table entry 0 and samples the frame at (0, 0), as a rebuilt handle does.
#pragma once
#include "bevw_device.h"
#include "bevw_moving.h"

namespace bevw {

// two taps of one map row in one load: 8 bytes of und1 at a 4-byte boundary, 4 bytes of und2 at a 2-byte boundary
struct __attribute__((packed, aligned(4))) MovingTaps1 { int16_t v[4]; };    // x, y of tap 0; x, y of tap 1
struct __attribute__((packed, aligned(2))) MovingTaps2 { uint16_t v[2]; };

typedef const double __attribute__((address_space(4))) *moving_const_f64;   // the constant address space: scalar loads

// Step 2 for one camera: the BEV table entry (o1: top-left frame texel, o2: fraction code before its mask) at undistorted-grid position
// (sx, sy, code).  Interior footprints: remap_f32_px's expression on taps fetched pairwise; every other footprint: remap_f32_px itself.
__device__ __forceinline__ void moving_table_px(const int16_t *__restrict__ und1, const uint16_t *__restrict__ und2, int uw, int uh, int sx, int sy,
                                                unsigned code, bool classic2, int o1[2], int o2[1])
{
    const unsigned xlim = uw > 1 ? uw - 1 : 0, ylim = uh > 1 ? uh - 1 : 0;
    if ((unsigned)sx < xlim && (unsigned)sy < ylim) {
        const float fx = (float)(code & 31) * (1.f / 32), fy = (float)((code >> 5) & 31) * (1.f / 32);
        const float ax = 1.f - fx, ay = 1.f - fy;
        const float w0 = ay * ax, w1 = ay * fx, w2 = fy * ax, w3 = fy * fx;
        const size_t i = (size_t)sy * uw + sx;
        const MovingTaps1 r0 = *reinterpret_cast<const MovingTaps1 *>(und1 + i * 2), r1 = *reinterpret_cast<const MovingTaps1 *>(und1 + (i + uw) * 2);
#pragma unroll
        for (int k = 0; k < 2; ++k) o1[k] = rne_f((float)r0.v[k] * w0 + (float)r0.v[k + 2] * w1 + (float)r1.v[k] * w2 + (float)r1.v[k + 2] * w3);
        if (classic2) {
            const MovingTaps2 q0 = *reinterpret_cast<const MovingTaps2 *>(und2 + i), q1 = *reinterpret_cast<const MovingTaps2 *>(und2 + i + uw);
            o2[0] = rne_f((float)q0.v[0] * w0 + (float)q0.v[1] * w1 + (float)q1.v[0] * w2 + (float)q1.v[1] * w3);
        }
    } else {
        remap_f32_px<int16_t, 2>(und1, uw, uh, sx, sy, code, o1);
        if (classic2) remap_f32_px<uint16_t, 1>(und2, uw, uh, sx, sy, code, o2);
    }
}

// One block of 4 waves owns a 64 x 4 BEV tile (one wave per row, one lane per pixel) for the frame sets of its batch slice: mask bytes, blend
// weights and the car are read once, and consecutive frame sets hit nearly the same lines of the undistort maps.  The inverse of (frame set,
// camera) is uniform over the block and read through the constant address space.  A camera whose mask byte is 0 is skipped before any
// arithmetic.  No LDS, no barrier.
template <bool BLEND>
__global__ void __launch_bounds__(256) k_stitch_moving(MovingArgs a)
{
    const int x = blockIdx.x * kMovingTileW + (threadIdx.x & 63), y = blockIdx.y * kMovingTileH + (threadIdx.x >> 6);
    if (x >= a.bw || y >= a.bh) return;
    const size_t o = (size_t)y * a.bw + x;
    int m[4], car[3] = {0, 0, 0};
    float wgt[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        m[c] = a.mask[c][o];
        wgt[c] = blend_weight_f32(m[c]);
    }
    if (a.car != nullptr) { car[0] = a.car[o * 3]; car[1] = a.car[o * 3 + 1]; car[2] = a.car[o * 3 + 2]; }
    const bool classic2 = !(a.warp_mode & kWarpF32);
    const size_t frame_bytes = (size_t)a.fw * a.fh * 3, img_bytes = (size_t)a.pitch * a.bh * 3;
    const int b_begin = (int)blockIdx.z * a.nb, b_end = min(a.batch, b_begin + a.nb);
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (m[c] == 0) continue;
            const moving_const_f64 mc = (moving_const_f64)(a.minv + ((size_t)b * 4 + c) * 9);
            double M[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = mc[k];
            int sx, sy, o1[2], o2[1];
            unsigned code;
            perspective_coord(M, x, y, a.bw0, sx, sy, code);
            moving_table_px(a.und1[c], a.und2[c], a.uw, a.uh, sx, sy, code, classic2, o1, o2);
            if (!classic2) warp_f32_px<uint16_t, 1>(a.und2[c], a.uw, a.uh, M, x, y, a.warp_mode, o2);
            int v[3];
            remap_u8c3_px<false>(a.frames + ((size_t)b * 4 + c) * frame_bytes, a.fw, a.fh, (int)(int16_t)sat_s16(o1[0]), (int)(int16_t)sat_s16(o1[1]),
                                 (unsigned)(uint16_t)sat_u16(o2[0]) & (kQTab2 - 1), v, 0, nullptr, a.ties_even);
            if (BLEND) { v[0] = blend_mul(v[0], wgt[c]); v[1] = blend_mul(v[1], wgt[c]); v[2] = blend_mul(v[2], wgt[c]); }
            acc[0] = min(255, acc[0] + v[0]); acc[1] = min(255, acc[1] + v[1]); acc[2] = min(255, acc[2] + v[2]);
        }
        uint8_t *d = a.out + (size_t)b * img_bytes + ((size_t)y * a.pitch + x) * 3;
        d[0] = (uint8_t)min(255, acc[0] + car[0]); d[1] = (uint8_t)min(255, acc[1] + car[1]); d[2] = (uint8_t)min(255, acc[2] + car[2]);
    }
}

}  // namespace bevw
