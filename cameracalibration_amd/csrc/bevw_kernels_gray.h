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
// plan_unit_run (bevw_unit.h) for one channel: one block of 4 waves owns a unit for the frames of its batch chunk.  Per frame every lane
// fetches up to GR group slots -- ONE 8-byte load each at the slot's 4-byte aligned offset (unit_gsrc_gray) through the frame set's
// range-checked descriptor, as the NV12 unit kernel fetches its Y bytes.  Only the last group of the set's last row would reach a dword
// past the set (it would read as zero and touch nothing), and the plan never hands that group to a unit: unit_compile drops every base
// tile whose 16-byte BGR window would overrun the frame set, which is that group's (tests/test_gray_host.py holds it on a map that ends
// in the frame's last texel).  Texel 4g+4 of a row's last group is never sampled either (its footprint would cross the frame border: a
// base tile of the per-tap kernel).  A lane without a group is out of the descriptor's range as a whole.  The 8 bytes go to the
// patch half of their frame as they are.  The groups of the next two frames are in flight in registers; frame b+1 lands in the other
// half while frame b is interpolated: one barrier per frame for every class (GR x 2 KB per half).
// Single-contributor classes only (a one-camera plan has no other: plan_make_lists refuses the list otherwise): no blend, no channel
// sums, no car sprite, no wide fractions.
template <int NQ, int GR>
__device__ __forceinline__ void gray_unit_run(const PlanArgs &a, uint32_t chunk, uint32_t unit, uint8_t *lds)
{
    static_assert(NQ >= 1 && NQ <= kUnitMaxNQ && GR >= 1 && GR <= kUnitMaxGR, "unit class");
    constexpr int kPatch = GR * kUnitThreads * kGraySlotBytes;
    static_assert(2 * kPatch <= 2 * kGrayPatch, "both halves of the frame ring fit the block's LDS");
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(a.un_desc + unit);
    const uint32_t pos = __builtin_amdgcn_readfirstlane(dp[0]), shape = __builtin_amdgcn_readfirstlane(dp[1]);
    const uint32_t ent_off = __builtin_amdgcn_readfirstlane(dp[2]), gs_off = __builtin_amdgcn_readfirstlane(dp[3]);
    const uint32_t lq = __builtin_amdgcn_readfirstlane(dp[4]);
    const uint32_t ngroups = __builtin_amdgcn_readfirstlane(dp[6]);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ux = (int)(int16_t)(pos & 0xffffu), uy = (int)(pos >> 16), uw = (int)(shape & 0xffffu), uh = (int)(shape >> 16);
    const size_t set_bytes = a.set_stride ? (size_t)a.set_stride : (size_t)a.fw * a.fh * a.ncams, img_bytes = (size_t)a.pitch * a.bh;
    const bool streaming = (uint32_t)a.pitch % 64u == 0u;   // rows of whole sectors (unit_store_quad's rule)

    uint32_t a0[NQ][4], a1[NQ][4], pk[NQ][4], wx[NQ][4], wy[NQ][4], gs[GR], ooff[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int sidx = unit_slot(wave, j);
        int qx, row;
        unit_quad(lq, sidx, lane, qx, row);
        const int x = ux + 4 * qx + unit_skew((uint32_t)a.un_skew, uy + row);
        const uint4 e4 = unit_plan_load(a.un_entries + ((size_t)ent_off + sidx) * 64 + lane);   // the lane's 4 pixels of this slot
        const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) gray_decode(e[p], a0[j][p], a1[j][p], pk[j][p], wx[j][p], wy[j][p]);
        const bool store = 4 * qx < uw && row < uh && x >= 0 && x < a.pitch && !(unit_no_contributor(e[0]) && (e[0] & kUnitSkip));
        // out of range of the image's buffer descriptor: not written
        ooff[j] = store ? (uint32_t)(uy + row) * (uint32_t)a.pitch + (uint32_t)x : kPairNoGroup;
    }
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
    auto frame_of = [&](int b) { return min(b, b_end - 1); };   // past the chunk: the last frame once more
    auto image = [&](int b) { return __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)frame_of(b) * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3); };

    if (ngroups == 0) {
        // no contributor anywhere (the map leaves the frame): zeros, in whole row runs
#pragma unroll 1
        for (int b = b_begin; b < b_end; ++b) {
            const __amdgpu_buffer_rsrc_t ro = image(b);
#pragma unroll
            for (int j = 0; j < NQ; ++j) unit_store_dword(0u, ro, (int)ooff[j], streaming);
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < GR; ++r) gs[r] = once_load<BEVW_PLAN_NT>(a.un_gsrc + ((size_t)gs_off + r) * kUnitThreads + threadIdx.x);

    pair_u32x2 pf[2][GR];
    auto issue = [&](int b, int ring) {
        const uint8_t *src = a.frames + (size_t)frame_of(b) * set_bytes;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src), 0, (uint32_t)set_bytes, kBufferWord3);
#pragma unroll
        for (int r = 0; r < GR; ++r) pf[ring][r] = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)gs[r], 0, kPairLoadAux);
    };
    auto land = [&](int ring) {   // the groups of ring slot `ring` -> the patch half of that frame: 8 bytes per group slot, as fetched
#pragma unroll
        for (int r = 0; r < GR; ++r)
            reinterpret_cast<uint2 *>(lds + ring * kPatch)[r * kUnitThreads + (int)threadIdx.x] = make_uint2(pf[ring][r].x, pf[ring][r].y);
    };
    auto frame = [&](int b, int ring) {
        const uint8_t *const pw = lds + ring * kPatch;
        issue(b + 2, ring);        // the ring slot of frame b has landed
        uint32_t d[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            uint32_t acc[4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
                acc[p] = gray_pixel(*reinterpret_cast<const uint2 *>(pw + a0[j][p]), *reinterpret_cast<const uint2 *>(pw + a1[j][p]), pk[j][p], wx[j][p], wy[j][p]);
            d[j] = gray_pack(acc);
        }
        land(ring ^ 1);            // frame b+1 into the other half: nobody reads it before the barrier
        const __amdgpu_buffer_rsrc_t ro = image(b);   // past the chunk: re-writes the last frame with the same bytes
#pragma unroll
        for (int j = 0; j < NQ; ++j) unit_store_dword(d[j], ro, (int)ooff[j], streaming);
        block_lds_barrier();       // half[ring ^ 1] complete for everybody, half[ring] free for frame b+2
    };
    issue(b_begin, 0);
    issue(b_begin + 1, 1);
    land(0);
    block_lds_barrier();
#pragma unroll 1
    for (int b = b_begin; b < b_end; b += 2) {
        frame(b, 0);
        frame(b + 1, 1);
    }
}

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
#define BEVW_GRAY_CASE(C) case C: static_assert(kUnitClassCON[C] == 1, "one contributor per pixel"); gray_unit_run<kUnitClassNQ[C], kUnitClassGR[C]>(a, chunk, unit, patch); break;
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
        unit_store_dword(d, ro, (int)((uint32_t)y * (uint32_t)a.pitch + (uint32_t)x0), false);
    }
}

// k_remap_lut on one-channel sources: one thread per destination pixel, both tie rules; grid = (ceil(dw / 256), dh, images)
__global__ void __launch_bounds__(256) k_remap_lut_gray(const uint8_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                       const uint16_t *__restrict__ map2, int dw, int dh, uint8_t *__restrict__ dst, int ties_even)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= dw) return;
    const size_t o = (size_t)y * dw + x;
    const uint8_t *s = src + (size_t)blockIdx.z * sw * sh;
    dst[(size_t)blockIdx.z * dw * dh + o] = (uint8_t)remap_u8c1_px(s, sw, sh, map1[o * 2], map1[o * 2 + 1], map2[o] & (kQTab2 - 1), ties_even);
}
#endif   // BEVW_GRAY_SHARED_ONLY

}  // namespace bevw
