// bevw_kernels_gray.h -- every kernel that reads one-channel frames (bevw_remapper_set_channels: 8UC1 sources and destinations of a
// remapper), under names of their own.  Included by bevwarp_gray.hip, behind bevw_plan.h with BEVW_PLAN_SHARED_ONLY (and by
// tests/native/gray_emulate.cpp, which runs the __host__ __device__ functions below on a CPU); bevw_kernels_gray_stitch.h, the one-channel
// stitch of a handle, includes it with BEVW_GRAY_SHARED_ONLY for the lane and device functions alone.
//
// The plan is the three-channel remapper's: the same unit partition, the same entries (pair index, two group slots, fx, fy), the same
// launch order.  What differs is what a group slot holds.  A group is texels 4g .. 4g+4 of one source row; in one channel those are the
// bytes 4g .. 4g+4 of the frame set, and pair p of the group (texels 4g+p, 4g+p+1) is bytes p, p+1 of the 8 bytes at offset 4g: the
// slot's 8-byte load IS its four pair entries, and nothing is converted where it lands.  The LDS patch is 8 bytes per slot (8 KB for a
// 1024-group unit against 32 KB in three channels), so both halves of the frame ring fit for every unit class.  A pixel reads the 8 bytes
// of its two slots (ds_read_b64, 8-byte aligned), shifts its pair to byte 0 (v_alignbyte_b32) and interpolates with the three-channel
// kernel's per-channel arithmetic: (sum p * w + 512) >> 10 in the separable form, exact in integers, ties half up.  A lane's quad is 4
// bytes: one dword store per quad slot.
#pragma once
#include "bevw_plan.h"
#include "bevw_mono_unit.h"

namespace bevw {

constexpr int kGraySlotBytes = 8;                                  // LDS bytes per group slot: texels 4g .. 4g+7, of which 4g .. 4g+4 are used
constexpr int kGrayPatch = kUnitMaxGroups * kGraySlotBytes;        // the largest unit's patch of one frame; the block holds two

// one plan entry (unit_entry) -> the LDS byte offsets of its two slots inside a frame's patch, its pair, x weights {32 - fx, fx, 0, 0}
// (zero for a pixel without a contributor: equal slots), y weights x 64 as unit_decode makes them
__host__ __device__ __forceinline__ void gray_decode(uint32_t e, uint32_t &a0, uint32_t &a1, uint32_t &k, uint32_t &wx, uint32_t &wy)
{
    const uint32_t s0 = (e >> 2) & 1023u, s1 = (e >> 12) & 1023u, fx = (e >> 22) & 31u, fy = e >> 27;
    a0 = s0 * (uint32_t)kGraySlotBytes;
    a1 = s1 * (uint32_t)kGraySlotBytes;
    k = e & 3u;
    wx = s0 != s1 ? ((32u - fx) | (fx << 8)) : 0u;
    wy = ((32u - fy) << 6) | (fy << 22);
}
// one pixel from the 8 bytes of its two slots: accumulator with the result byte in bits 16..23 (bilinear_pairs' form for one channel)
__host__ __device__ __forceinline__ uint32_t gray_pixel(uint2 q0, uint2 q1, uint32_t k, uint32_t wx, uint32_t wy64)
{
    const uint32_t t0 = px_alignbyte(q0.y, q0.x, k), t1 = px_alignbyte(q1.y, q1.x, k);   // bytes k, k+1 of the slot in bytes 0, 1
    const uint32_t h0 = px_dot4(t0, wx, 0u), h1 = px_dot4(t1, wx, 0u);                   // <= 255 * 32
    return px_dot2(h0 | (h1 << 16), wy64, 32768u);
}
// the accumulators of a lane's 4 pixels -> its dword
__host__ __device__ __forceinline__ uint32_t gray_pack(const uint32_t acc[4])
{
    return px_perm(acc[1], acc[0], 0x0c0c0602u) | px_perm(acc[3], acc[2], 0x06020c0cu);
}

// ---- the unit kernel ------------------------------------------------------------------------------------------------------------------
// mono_unit_run (bevw_mono_unit.h) has the loop, the frame ring and the end-of-set argument; here is what 1-byte texels give it.
//
// The group slots of 1-byte texels, shared with the one-channel stitch (bevw_kernels_gray_stitch.h): the patch, the fetch and the landing --
// ONE 8-byte load per group slot, landed in the patch half of its frame as fetched
template <int GR>
struct GraySlots {
    static constexpr int kGR = GR, kTexelBytes = 1, kPatch = GR * kUnitThreads * kGraySlotBytes, kMaxPatch = kGrayPatch;
    typedef pair_u32x2 Fetch;
    static __device__ __forceinline__ uint32_t group_offset(uint32_t g) { return g; }
    static __device__ __forceinline__ Fetch fetch(__amdgpu_buffer_rsrc_t rs, int off) { return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, kPairLoadAux); }
    static __device__ __forceinline__ void land(uint8_t *half, int idx, Fetch f) { reinterpret_cast<uint2 *>(half)[idx] = make_uint2(f.x, f.y); }
};
// The lane of the one-channel remapper, fixed-point bilinear weights: per frame a pixel reads the 8 bytes of its two slots and interpolates
// (gray_pixel), and a lane's 4 pixels are one dword.  Single-contributor classes only (a one-camera plan has no other: plan_make_lists
// refuses the list otherwise): no blend, no channel sums, no car sprite, no wide fractions.
template <int NQ, int GR>
struct GrayLane : GraySlots<GR> {
    static constexpr int kNQ = NQ, kPart = 1;
    typedef uint32_t Quad;
    uint32_t a0[NQ][4], a1[NQ][4], pk[NQ][4], wx[NQ][4], wy[NQ][4];

    __device__ __forceinline__ uint32_t load(int j, const uint4 *ent)
    {
        const uint4 e4 = unit_plan_load(ent);
        const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) gray_decode(e[p], a0[j][p], a1[j][p], pk[j][p], wx[j][p], wy[j][p]);
        return e[0];
    }
    __device__ __forceinline__ void place(int, bool, int, int) {}
    __device__ __forceinline__ void ready() {}
    __device__ __forceinline__ Quad empty(int) const { return 0u; }   // the map leaves the frame: zeros
    __device__ __forceinline__ Quad quad(int j, const uint8_t *pw) const
    {
        uint32_t acc[4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
            acc[p] = gray_pixel(*reinterpret_cast<const uint2 *>(pw + a0[j][p]), *reinterpret_cast<const uint2 *>(pw + a1[j][p]), pk[j][p], wx[j][p], wy[j][p]);
        return gray_pack(acc);
    }
};

// BEVW_GRAY_SHARED_ONLY (bevwarp_gray_stitch.hip): this header without its kernels -- the lane functions and device functions only.  A
// non-template kernel is emitted by every unit that sees it.
#ifndef BEVW_GRAY_SHARED_ONLY
// every unit of every class in the partition's own order, one launch per step: plan_unit_any's block map and class switch over the
// single-contributor classes
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_units_gray(PlanArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[2 * kGrayPatch];
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    if ((int)group >= a.nlist) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(a.tile_list[group]), unit = e & 0x0fffffffu;
#define BEVW_GRAY_CASE(C) case C: { static_assert(kUnitClassCON[C] == 1, "one contributor per pixel"); GrayLane<kUnitClassNQ[C], kUnitClassGR[C]> ln; mono_unit_run(a, ln, chunk, unit, patch); } break;
    switch (e >> 28) {
        BEVW_GRAY_CASE(0) BEVW_GRAY_CASE(1) BEVW_GRAY_CASE(2) BEVW_GRAY_CASE(3) BEVW_GRAY_CASE(7)
        default: break;   // (two-contributor classes: the host makes no one-channel list for a plan that has such units)
    }
#undef BEVW_GRAY_CASE
}
#endif   // BEVW_GRAY_SHARED_ONLY

// ---- the per-tap and per-pixel kernels ------------------------------------------------------------------------------------------------------
// cv2.remap u8c1, INTER_LINEAR fixed point, BORDER_CONSTANT 0: remap_u8c3_px (bevw_device.h) for one channel, one path for interior and
// border footprints -- a tap outside the frame is 0
__device__ __forceinline__ int remap_u8c1_px(const uint8_t *__restrict__ src, int sw, int sh, int sx, int sy, unsigned code, int ties_even)
{
    if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) return 0;
    const int fx = code & 31, fy = (code >> 5) & 31;
    const int ax = kQOne - fx, ay = kQOne - fy;
    int t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = sx + (q & 1), y = sy + (q >> 1);
        t[q] = ((unsigned)x < (unsigned)sw && (unsigned)y < (unsigned)sh) ? (int)src[(size_t)y * sw + x] : 0;
    }
    return remap_round10(t[0] * (ax * ay) + t[1] * (fx * ay) + t[2] * (ax * fy) + t[3] * (fx * fy), ties_even);
}

#ifndef BEVW_GRAY_SHARED_ONLY
// The per-tap tile kernel on one-channel frames: one wave per 32 x 8 base tile of the list (the tiles no unit owns: footprints on the frame
// border), lane l owns the pixel quad (l % 8, l / 8), every tap read straight from the frame.  k_stitch_plan's block map and entries; an
// entry without a contributor gives 0.  Rows of a.pitch == a.bw bytes, a.bw % 4 == 0: one dword store per lane.
// (mono_tiles of bevw_mono_unit.h is this walk for the nearest kernels.  This kernel and k_stitch_plan_gray16 keep their own text: they
// take the kernel's arguments directly, and already passing them to a shared body by reference changes their machine code.)
__global__ void __launch_bounds__(256) k_stitch_plan_gray(PlanArgs a)
{
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    const int lane = threadIdx.x & 63;
    const int slot = (int)group * (int)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (slot >= a.nlist) return;
    const int tile = a.tile_list ? (int)__builtin_amdgcn_readfirstlane(a.tile_list[slot]) : slot;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x0 = (tx * kPlanLX + lane % kPlanLX) * 4, y = ty * kPlanLY + lane / kPlanLX;
    if (x0 >= a.bw || y >= a.bh) return;
    const size_t set_bytes = (size_t)a.fw * a.fh * a.ncams, img_bytes = (size_t)a.pitch * a.bh;
    EntryRegs e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e[j] = decode_entry(a.plan[((size_t)tile * 8 + j) * 64 + lane], false);
        entry_to_taps(e[j], a.fw, (uint32_t)a.fw * a.fh * 3);   // (the plan's interior entries hold BGR frame-set offsets)
    }
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const uint8_t *fb = a.frames + (size_t)b * set_bytes;
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(e[j].meta & kMetaValid)) continue;
            const int cam = (e[j].meta >> 18) & 3, sx = (int)(int16_t)(e[j].off & 0xffffu), sy = (int)(int16_t)(e[j].off >> 16);
            d |= (uint32_t)remap_u8c1_px(fb + (size_t)cam * a.fw * a.fh, a.fw, a.fh, sx, sy, e[j].meta & 1023u, 0) << (8 * j);
        }
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3);
        mono_store(d, ro, (int)((uint32_t)y * (uint32_t)a.pitch + (uint32_t)x0), false);
    }
}

// k_remap_lut on one-channel sources (mono_remap), both tie rules
__global__ void __launch_bounds__(256) k_remap_lut_gray(const uint8_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                       const uint16_t *__restrict__ map2, int dw, int dh, uint8_t *__restrict__ dst, int ties_even)
{
    mono_remap<uint8_t>(src, sw, sh, map1, map2, dw, dh, dst, [ties_even](const uint8_t *s, int w, int h, int sx, int sy, unsigned code) {
        return remap_u8c1_px(s, w, h, sx, sy, code, ties_even);
    });
}
#endif   // BEVW_GRAY_SHARED_ONLY

}  // namespace bevw
