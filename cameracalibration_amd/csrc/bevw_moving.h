// bevw_moving.h -- the launcher of the stitch with a homography per frame set (bevw_run_homographies_device: moving extrinsics).  Its kernel
// has a name of its own (k_stitch_moving: bevw_kernels_moving.h) and is compiled in bevwarp_moving.hip alone, which defines the function
// declared here; the main unit's entry points call it.  The launcher queues its kernel on `st`; the caller reads hipGetLastError() as after
// its own launches.
#pragma once
#include "bevw_host.h"

namespace bevw {

// One batch chunk of a moving step.  Frame set b of the chunk is stitched through the BEV tables cv2.warpPerspective(undistort maps, H_b)
// would hold, evaluated per pixel from the handle's resident undistort maps: nothing is written but the images.
struct MovingArgs {
    const uint8_t *frames;     // [batch][4][fh][fw][3], dense BGR, any alignment
    const double *minv;        // [batch][4][9]: the INVERSE of every homography (invert3x3 on the host), device memory
    const int16_t *und1[4];    // the undistort maps of the four cameras: [uh][uw][2] top-left texels ...
    const uint16_t *und2[4];   // ... and [uh][uw] fraction codes
    const uint8_t *mask[4];    // [bh][bw]: the direct masks or the blend weights
    const uint8_t *car;        // [bh][bw][3] dense, or nullptr
    uint8_t *out;              // [batch][bh][pitch][3], any alignment
    int fw, fh, uw, uh, bw, bh;
    int bw0;                   // persp_block_width(bw, bh): the column blocks of cv2.warpPerspective
    int pitch;                 // pixels per row of an image
    int batch;                 // frame sets of the chunk
    int nb;                    // frame sets per block: block z of the grid owns [z * nb, min(batch, (z + 1) * nb))
    int warp_mode;             // the handle's BEVW_COMPAT_WARP (k_bev_lut's)
    int ties_even;             // the handle's BEVW_COMPAT_REMAP (remap_u8c3_px's)
};

constexpr int kMovingTileW = 64, kMovingTileH = 4;   // the BEV tile of a block: one wave per row

// frame sets per block for a chunk of `batch` sets on `tiles` BEV tiles: as many as leave the launch at least kMovingMinBlocks blocks, 16
// at the most (consecutive frame sets of a block then hit nearly the same lines of the undistort maps)
constexpr int kMovingMinBlocks = 4096;
inline int moving_nb(int batch, long long tiles)
{
    int nb = 16;
    while (nb > 1 && tiles * ((batch + nb - 1) / nb) < kMovingMinBlocks) nb /= 2;
    return nb;
}

// k_stitch_moving<blend> over the chunk: grid (ceil(bw / 64), ceil(bh / 4), ceil(batch / nb))
void moving_launch_stitch(hipStream_t st, const MovingArgs &a, bool blend);

}  // namespace bevw
