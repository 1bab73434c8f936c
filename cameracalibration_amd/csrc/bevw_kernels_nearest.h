// bevw_kernels_nearest.h -- every kernel of a one-channel remapper in nearest-neighbour mode (bevw_remapper_set_interpolation:
// cv2.remap(..., cv2.INTER_NEAREST) on class-ID maps, instance-ID maps and masks), at 8 and at 16 bits, under names of their own.  Included
// by bevwarp_nearest.hip behind bevw_plan.h with BEVW_PLAN_SHARED_ONLY and bevw_kernels_gray.h with BEVW_GRAY_SHARED_ONLY (and by
// tests/native/nearest_emulate.cpp, which runs the __host__ __device__ functions below on a CPU).
//
// The rule.  With fixed-point maps (map1 CV_16SC2, map2 CV_16UC1) cv2's nearest texel is a pure function of them: a = map2 & 1023,
// fx = a & 31, fy = a >> 5, x = (short)(map1.x + (fx >= 16)), y = (short)(map1.y + (fy >= 16)), dst = src[y][x] inside the frame and 0
// outside.  No rounding, no tie rule, no depth-dependent arithmetic; BEVW_COMPAT_REMAP has nothing to select.  The sum wraps in a short
// (32767 + 1 -> -32768), which only a source wider or higher than 32768 can show: those remappers never take the plan (bevwarp.hip).
//
// The plan is the one-channel remapper's: the same unit partition, entries (pair index k, group slots s0 / s1 of footprint rows sy / sy + 1,
// fx, fy), launch order and group list.  A unit stages every texel one of its pixels could pick: the nearest texel is texel k + (fx >= 16)
// of the group in slot (fy >= 16 ? s1 : s0).  So before the frame loop a pixel is reduced to ONE LDS byte address, and per frame it is one
// ds_read_u8 / ds_read_u16; a pixel without a contributor (equal slots) reads address 0 and is masked to zero with its quad (one AND per
// dword).  A quad is one dword store at 8 bits and one 8-byte store at 16.
//
// LDS.  8 bits: a group's 8 fetched bytes land as they are, 8 bytes per slot (bevw_kernels_gray.h); texel t = 0 .. 4 of slot s is byte
// 8 s + t.  16 bits: a group is ONE 12-byte load {d0, d1, d2} = texels 4g .. 4g+5 (bevw_kernels_gray16.h has why the third dword never
// straddles the end of a frame set); {d0, d1} land in plane 0 at 8 bytes per slot and d2 in plane 1 at 4 bytes per slot, so texel t <= 3
// is the aligned 2 bytes at 8 s + 2 t of plane 0 and texel 4 the 2 bytes at 4 s of plane 1: 12 KB per frame for a 1024-group unit, 24 KB
// for the two halves of the frame ring (16 KB at 8 bits).  Consecutive slots stay 8 (4) bytes apart, as in the linear kernels: the lanes of
// a read group that walk consecutive slots spread over the bank row.
#pragma once
#include <type_traits>

#include "bevw_plan.h"
#include "bevw_kernels_gray.h"

namespace bevw {

constexpr int kNearestSlotBytes8 = kGraySlotBytes;                              // 8 bits: LDS bytes per group slot
constexpr int kNearestPatch8 = kUnitMaxGroups * kNearestSlotBytes8;             // the largest unit's patch of one frame; the block holds two
constexpr int kNearestPlane0Bytes16 = 8, kNearestPlane1Bytes16 = 4;             // 16 bits: LDS bytes per group slot in plane 0 (texels 0 .. 3) and plane 1 (texels 4, 5)
constexpr int kNearestPatch16 = kUnitMaxGroups * (kNearestPlane0Bytes16 + kNearestPlane1Bytes16);
constexpr uint32_t kNearestNone = 0xffffffffu;                                  // nearest_decode*: the pixel has no contributor

// cv2's NNDeltaTab_i: the step from a footprint's first texel to its nearest one
__host__ __device__ __forceinline__ uint32_t nearest_dx(uint32_t code) { return (code >> 4) & 1u; }   // fx >= 16
__host__ __device__ __forceinline__ uint32_t nearest_dy(uint32_t code) { return (code >> 9) & 1u; }   // fy >= 16

// one plan entry (unit_entry) -> the LDS byte offset of its nearest texel inside a frame's patch, or kNearestNone (equal slots)
__host__ __device__ __forceinline__ uint32_t nearest_decode8(uint32_t e)
{
    const uint32_t k = e & 3u, s0 = (e >> 2) & 1023u, s1 = (e >> 12) & 1023u, code = e >> 22;
    if (s0 == s1) return kNearestNone;
    return (nearest_dy(code) ? s1 : s0) * (uint32_t)kNearestSlotBytes8 + k + nearest_dx(code);
}
// ... at 16 bits; plane0_bytes = the bytes of plane 0 of the unit's patch (its slots x 8)
__host__ __device__ __forceinline__ uint32_t nearest_decode16(uint32_t e, uint32_t plane0_bytes)
{
    const uint32_t k = e & 3u, s0 = (e >> 2) & 1023u, s1 = (e >> 12) & 1023u, code = e >> 22;
    if (s0 == s1) return kNearestNone;
    const uint32_t s = nearest_dy(code) ? s1 : s0, t = k + nearest_dx(code);
    return t < 4u ? s * (uint32_t)kNearestPlane0Bytes16 + 2u * t : plane0_bytes + s * (uint32_t)kNearestPlane1Bytes16;
}
// a lane's 4 texels -> its store, under the quad's mask (0 in the bytes of a pixel without a contributor)
__host__ __device__ __forceinline__ uint32_t nearest_pack8(const uint32_t v[4], uint32_t mask)
{
    return (v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24)) & mask;
}
__host__ __device__ __forceinline__ uint2 nearest_pack16(const uint32_t v[4], uint2 mask)
{
    return make_uint2((v[0] | (v[1] << 16)) & mask.x, (v[2] | (v[3] << 16)) & mask.y);
}
// the pick of the per-tap and per-pixel kernels, with its own range check: sx, sy = map1 (or the plan entry's), code = map2 & 1023.
// The sum is cv2's short.
template <typename T>
__host__ __device__ __forceinline__ uint32_t nearest_px(const T *__restrict__ src, int sw, int sh, int sx, int sy, uint32_t code)
{
    const int x = (int)(int16_t)(sx + (int)nearest_dx(code)), y = (int)(int16_t)(sy + (int)nearest_dy(code));
    return ((unsigned)x < (unsigned)sw && (unsigned)y < (unsigned)sh) ? (uint32_t)src[(size_t)y * sw + x] : 0u;
}

// ---- the unit kernels ---------------------------------------------------------------------------------------------------------------------
// The lane of mono_unit_run (bevw_mono_unit.h has the loop and the frame ring) with the rule above: per frame every lane fetches up to GR
// group slots (8 or 12 bytes each; the offsets of the one-channel list, doubled at 16 bits) and a pixel is one LDS read at the address
// worked out before the frame loop.  Single-contributor classes only.
template <int DEPTH, int NQ, int GR>
struct NearestLane {
    static_assert(DEPTH == 8 || DEPTH == 16, "bits per texel");
    static constexpr bool DEEP = DEPTH == 16;
    static constexpr int kNQ = NQ, kGR = GR, kTexelBytes = DEPTH / 8, kPart = 1;
    static constexpr int kPlane0 = GR * kUnitThreads * (DEEP ? kNearestPlane0Bytes16 : kNearestSlotBytes8);
    static constexpr int kPatch = kPlane0 + (DEEP ? GR * kUnitThreads * kNearestPlane1Bytes16 : 0), kMaxPatch = DEEP ? kNearestPatch16 : kNearestPatch8;
    typedef std::conditional_t<DEEP, uint2, uint32_t> Quad;
    typedef std::conditional_t<DEEP, pair_u32x3, pair_u32x2> Fetch;
    uint32_t ad[NQ][4];
    Quad mask[NQ];   // 0 in the bytes of a pixel without a contributor

    __device__ __forceinline__ uint32_t load(int j, const uint4 *ent)
    {
        const uint4 e4 = unit_plan_load(ent);
        const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
        uint32_t live[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t d = DEEP ? nearest_decode16(e[p], (uint32_t)kPlane0) : nearest_decode8(e[p]);
            live[p] = d != kNearestNone ? 1u : 0u;
            ad[j][p] = live[p] ? d : 0u;
        }
        if constexpr (DEEP) mask[j] = make_uint2(live[0] * 0xffffu | live[1] * 0xffff0000u, live[2] * 0xffffu | live[3] * 0xffff0000u);
        else mask[j] = live[0] * 0xffu | live[1] * 0xff00u | live[2] * 0xff0000u | live[3] * 0xff000000u;
        return e[0];
    }
    __device__ __forceinline__ void place(int, bool, int, int) {}
    __device__ __forceinline__ void ready() {}
    __device__ __forceinline__ Quad empty(int) const { return Quad(); }   // the map leaves the frame: zeros
    // (2 bytes per texel: twice the offset; the sentinel stays out of range)
    static __device__ __forceinline__ uint32_t group_offset(uint32_t g) { return DEEP ? (g == kPairNoGroup ? kPairNoGroup : g * 2u) : g; }
    static __device__ __forceinline__ Fetch fetch(__amdgpu_buffer_rsrc_t rs, int off)
    {
        if constexpr (DEEP) return __builtin_amdgcn_raw_buffer_load_b96(rs, off, 0, kPairLoadAux);
        else return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, kPairLoadAux);
    }
    static __device__ __forceinline__ void land(uint8_t *half, int idx, Fetch f)
    {
        reinterpret_cast<uint2 *>(half)[idx] = make_uint2(f.x, f.y);
        if constexpr (DEEP) reinterpret_cast<uint32_t *>(half + kPlane0)[idx] = f.z;
    }
    __device__ __forceinline__ Quad quad(int j, const uint8_t *pw) const
    {
        uint32_t v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = DEEP ? (uint32_t)*reinterpret_cast<const uint16_t *>(pw + ad[j][p]) : (uint32_t)pw[ad[j][p]];
        if constexpr (DEEP) return nearest_pack16(v, mask[j]);
        else return nearest_pack8(v, mask[j]);
    }
};

// every unit of every class in the partition's own order, one launch per step: k_units_gray's block map and class switch
template <int DEPTH>
__device__ __forceinline__ void nearest_units(const PlanArgs &a, uint8_t *patch)
{
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    if ((int)group >= a.nlist) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(a.tile_list[group]), unit = e & 0x0fffffffu;
#define BEVW_NEAREST_CASE(C) case C: { static_assert(kUnitClassCON[C] == 1, "one contributor per pixel"); NearestLane<DEPTH, kUnitClassNQ[C], kUnitClassGR[C]> ln; mono_unit_run(a, ln, chunk, unit, patch); } break;
    switch (e >> 28) {
        BEVW_NEAREST_CASE(0) BEVW_NEAREST_CASE(1) BEVW_NEAREST_CASE(2) BEVW_NEAREST_CASE(3) BEVW_NEAREST_CASE(7)
        default: break;   // (two-contributor classes: the host makes no one-channel list for a plan that has such units)
    }
#undef BEVW_NEAREST_CASE
}
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_units_nn8(PlanArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[2 * kNearestPatch8];
    nearest_units<8>(a, patch);
}
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_units_nn16(PlanArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[2 * kNearestPatch16];
    nearest_units<16>(a, patch);
}

// ---- the per-tap tile kernels and the per-pixel kernels -----------------------------------------------------------------------------------
// mono_tiles and mono_remap (bevw_mono_unit.h) over the pick: read straight from the frame with its own range check -- a pixel whose
// footprint straddles the border is its nearest texel where that lies inside -- and with the short's wrap
template <typename T>
struct NearestPx {
    __device__ __forceinline__ uint32_t operator()(const T *s, int sw, int sh, int sx, int sy, uint32_t code) const { return nearest_px<T>(s, sw, sh, sx, sy, code); }
};
__global__ void __launch_bounds__(256) k_tiles_nn8(PlanArgs a) { mono_tiles<uint8_t>(a, NearestPx<uint8_t>()); }
__global__ void __launch_bounds__(256) k_tiles_nn16(PlanArgs a) { mono_tiles<uint16_t>(a, NearestPx<uint16_t>()); }

__global__ void __launch_bounds__(256) k_remap_nn8(const uint8_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                  const uint16_t *__restrict__ map2, int dw, int dh, uint8_t *__restrict__ dst)
{
    mono_remap<uint8_t>(src, sw, sh, map1, map2, dw, dh, dst, NearestPx<uint8_t>());
}
__global__ void __launch_bounds__(256) k_remap_nn16(const uint16_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                   const uint16_t *__restrict__ map2, int dw, int dh, uint16_t *__restrict__ dst)
{
    mono_remap<uint16_t>(src, sw, sh, map1, map2, dw, dh, dst, NearestPx<uint16_t>());
}

}  // namespace bevw
