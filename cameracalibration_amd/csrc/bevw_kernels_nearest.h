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

// a lane's 16-bit quad: one 8-byte store under unit_store_dword's policy
__device__ __forceinline__ void nearest_store_qword(uint32_t lo, uint32_t hi, __amdgpu_buffer_rsrc_t ro, int off, bool streaming)
{
    const pair_u32x2 d = {lo, hi};
    if (streaming) __builtin_amdgcn_raw_buffer_store_b64(d, ro, off, 0, kPairStreamAux);
    else __builtin_amdgcn_raw_buffer_store_b64(d, ro, off, 0, kPairStoreAux);
}

// ---- the unit kernels ---------------------------------------------------------------------------------------------------------------------
// gray_unit_run (bevw_kernels_gray.h) / gray16_unit_run with the lane body of the rule above: one block of 4 waves owns a unit for the frames
// of its batch chunk; per frame every lane fetches up to GR group slots through the frame set's range-checked descriptor (8 or 12 bytes
// each; the offsets of the one-channel list, doubled at 16 bits), the groups of the next two frames are in flight in registers, frame b+1
// lands in the other half of the ring while frame b is picked: one barrier per frame.  Single-contributor classes only.
template <int DEPTH, int NQ, int GR>
__device__ __forceinline__ void nearest_unit_run(const PlanArgs &a, uint32_t chunk, uint32_t unit, uint8_t *lds)
{
    static_assert(DEPTH == 8 || DEPTH == 16, "bits per texel");
    static_assert(NQ >= 1 && NQ <= kUnitMaxNQ && GR >= 1 && GR <= kUnitMaxGR, "unit class");
    constexpr bool DEEP = DEPTH == 16;
    constexpr int BPP = DEPTH / 8;
    constexpr int kPlane0 = GR * kUnitThreads * (DEEP ? kNearestPlane0Bytes16 : kNearestSlotBytes8);
    constexpr int kPatch = kPlane0 + (DEEP ? GR * kUnitThreads * kNearestPlane1Bytes16 : 0);
    static_assert(2 * kPatch <= 2 * (DEEP ? kNearestPatch16 : kNearestPatch8), "both halves of the frame ring fit the block's LDS");
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(a.un_desc + unit);
    const uint32_t pos = __builtin_amdgcn_readfirstlane(dp[0]), shape = __builtin_amdgcn_readfirstlane(dp[1]);
    const uint32_t ent_off = __builtin_amdgcn_readfirstlane(dp[2]), gs_off = __builtin_amdgcn_readfirstlane(dp[3]);
    const uint32_t lq = __builtin_amdgcn_readfirstlane(dp[4]);
    const uint32_t ngroups = __builtin_amdgcn_readfirstlane(dp[6]);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ux = (int)(int16_t)(pos & 0xffffu), uy = (int)(pos >> 16), uw = (int)(shape & 0xffffu), uh = (int)(shape >> 16);
    const size_t set_bytes = a.set_stride ? (size_t)a.set_stride : (size_t)a.fw * a.fh * a.ncams * BPP, img_bytes = (size_t)a.pitch * a.bh * BPP;
    const bool streaming = ((uint32_t)a.pitch * (uint32_t)BPP) % 64u == 0u;   // rows of whole sectors (unit_store_quad's rule on bytes)

    uint32_t ad[NQ][4], mlo[NQ], mhi[NQ], gs[GR], ooff[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int sidx = unit_slot(wave, j);
        int qx, row;
        unit_quad(lq, sidx, lane, qx, row);
        const int x = ux + 4 * qx + unit_skew((uint32_t)a.un_skew, uy + row);
        const uint4 e4 = unit_plan_load(a.un_entries + ((size_t)ent_off + sidx) * 64 + lane);   // the lane's 4 pixels of this slot
        const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
        uint32_t live[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t d = DEEP ? nearest_decode16(e[p], (uint32_t)kPlane0) : nearest_decode8(e[p]);
            live[p] = d != kNearestNone ? 1u : 0u;
            ad[j][p] = live[p] ? d : 0u;
        }
        if (DEEP) {
            mlo[j] = live[0] * 0xffffu | live[1] * 0xffff0000u;
            mhi[j] = live[2] * 0xffffu | live[3] * 0xffff0000u;
        } else {
            mlo[j] = live[0] * 0xffu | live[1] * 0xff00u | live[2] * 0xff0000u | live[3] * 0xff000000u;
            mhi[j] = 0u;
        }
        const bool store = 4 * qx < uw && row < uh && x >= 0 && x < a.pitch && !(unit_no_contributor(e[0]) && (e[0] & kUnitSkip));
        // out of range of the image's buffer descriptor: not written
        ooff[j] = store ? ((uint32_t)(uy + row) * (uint32_t)a.pitch + (uint32_t)x) * (uint32_t)BPP : kPairNoGroup;
    }
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
    auto frame_of = [&](int b) { return min(b, b_end - 1); };   // past the chunk: the last frame once more
    auto image = [&](int b) { return __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)frame_of(b) * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3); };
    auto store_quad = [&](uint32_t lo, uint32_t hi, const __amdgpu_buffer_rsrc_t ro, int off) {
        if (DEEP) nearest_store_qword(lo, hi, ro, off, streaming);
        else unit_store_dword(lo, ro, off, streaming);
    };

    if (ngroups == 0) {
        // no contributor anywhere (the map leaves the frame): zeros, in whole row runs
#pragma unroll 1
        for (int b = b_begin; b < b_end; ++b) {
            const __amdgpu_buffer_rsrc_t ro = image(b);
#pragma unroll
            for (int j = 0; j < NQ; ++j) store_quad(0u, 0u, ro, (int)ooff[j]);
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        const uint32_t g = once_load<BEVW_PLAN_NT>(a.un_gsrc + ((size_t)gs_off + r) * kUnitThreads + threadIdx.x);
        gs[r] = DEEP ? (g == kPairNoGroup ? kPairNoGroup : g * 2u) : g;   // (2 bytes per texel: twice the offset; the sentinel stays out of range)
    }

    pair_u32x3 pf[2][GR];   // (8 bits: .z unused)
    auto issue = [&](int b, int ring) {
        const uint8_t *src = a.frames + (size_t)frame_of(b) * set_bytes;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src), 0, (uint32_t)set_bytes, kBufferWord3);
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            if (DEEP) pf[ring][r] = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)gs[r], 0, kPairLoadAux);
            else {
                const pair_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)gs[r], 0, kPairLoadAux);
                pf[ring][r].x = v.x; pf[ring][r].y = v.y;
            }
        }
    };
    auto land = [&](int ring) {   // the groups of ring slot `ring` -> the patch half of that frame
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            uint8_t *const half = lds + ring * kPatch;
            reinterpret_cast<uint2 *>(half)[r * kUnitThreads + (int)threadIdx.x] = make_uint2(pf[ring][r].x, pf[ring][r].y);
            if (DEEP) reinterpret_cast<uint32_t *>(half + kPlane0)[r * kUnitThreads + (int)threadIdx.x] = pf[ring][r].z;
        }
    };
    auto frame = [&](int b, int ring) {
        const uint8_t *const pw = lds + ring * kPatch;
        issue(b + 2, ring);        // the ring slot of frame b has landed
        uint32_t lo[NQ], hi[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            uint32_t v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
                v[p] = DEEP ? (uint32_t)*reinterpret_cast<const uint16_t *>(pw + ad[j][p]) : (uint32_t)pw[ad[j][p]];
            if (DEEP) {
                const uint2 q = nearest_pack16(v, make_uint2(mlo[j], mhi[j]));
                lo[j] = q.x; hi[j] = q.y;
            } else {
                lo[j] = nearest_pack8(v, mlo[j]); hi[j] = 0u;
            }
        }
        land(ring ^ 1);            // frame b+1 into the other half: nobody reads it before the barrier
        const __amdgpu_buffer_rsrc_t ro = image(b);   // past the chunk: re-writes the last frame with the same bytes
#pragma unroll
        for (int j = 0; j < NQ; ++j) store_quad(lo[j], hi[j], ro, (int)ooff[j]);
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

// every unit of every class in the partition's own order, one launch per step: k_units_gray's block map and class switch
template <int DEPTH>
__device__ __forceinline__ void nearest_units(const PlanArgs &a, uint8_t *patch)
{
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    if ((int)group >= a.nlist) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(a.tile_list[group]), unit = e & 0x0fffffffu;
#define BEVW_NEAREST_CASE(C) case C: static_assert(kUnitClassCON[C] == 1, "one contributor per pixel"); nearest_unit_run<DEPTH, kUnitClassNQ[C], kUnitClassGR[C]>(a, chunk, unit, patch); break;
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

// ---- the per-tap tile kernels -------------------------------------------------------------------------------------------------------------
// The base tiles no unit owns (footprints on the frame border): k_stitch_plan_gray's block map, entries and lane layout (one wave per 32 x 8
// base tile of the list, lane l owns the pixel quad (l % 8, l / 8)), the pick read straight from the frame with its own range check -- a
// pixel whose footprint straddles the border is its nearest texel where that lies inside.  Rows of a.pitch == a.bw pixels, a.bw % 4 == 0,
// a.out 4-byte aligned: one dword (8-byte) store per lane.
template <typename T>
__device__ __forceinline__ void nearest_tiles(const PlanArgs &a)
{
    constexpr int BPP = (int)sizeof(T);
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    const int lane = threadIdx.x & 63;
    const int slot = (int)group * (int)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (slot >= a.nlist) return;
    const int tile = a.tile_list ? (int)__builtin_amdgcn_readfirstlane(a.tile_list[slot]) : slot;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x0 = (tx * kPlanLX + lane % kPlanLX) * 4, y = ty * kPlanLY + lane / kPlanLX;
    if (x0 >= a.bw || y >= a.bh) return;
    const size_t set_texels = (size_t)a.fw * a.fh * a.ncams, img_bytes = (size_t)a.pitch * a.bh * BPP;
    EntryRegs e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e[j] = decode_entry(a.plan[((size_t)tile * 8 + j) * 64 + lane], false);
        entry_to_taps(e[j], a.fw, (uint32_t)a.fw * a.fh * 3);   // (the plan's interior entries hold BGR frame-set offsets)
    }
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
    const uint32_t off = ((uint32_t)y * (uint32_t)a.pitch + (uint32_t)x0) * (uint32_t)BPP;
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const T *fb = reinterpret_cast<const T *>(a.frames) + (size_t)b * set_texels;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(e[j].meta & kMetaValid)) continue;
            const int cam = (e[j].meta >> 18) & 3, sx = (int)(int16_t)(e[j].off & 0xffffu), sy = (int)(int16_t)(e[j].off >> 16);
            v[j] = nearest_px<T>(fb + (size_t)cam * a.fw * a.fh, a.fw, a.fh, sx, sy, e[j].meta & 1023u);
        }
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3);
        if (BPP == 2) {
            const uint2 q = nearest_pack16(v, make_uint2(~0u, ~0u));
            nearest_store_qword(q.x, q.y, ro, (int)off, false);
        } else unit_store_dword(nearest_pack8(v, ~0u), ro, (int)off, false);
    }
}
__global__ void __launch_bounds__(256) k_tiles_nn8(PlanArgs a) { nearest_tiles<uint8_t>(a); }
__global__ void __launch_bounds__(256) k_tiles_nn16(PlanArgs a) { nearest_tiles<uint16_t>(a); }

// ---- the per-pixel kernels ----------------------------------------------------------------------------------------------------------------
// one thread per destination pixel from map1 / map2, with the short's wrap; grid = (ceil(dw / 256), dh, images).  `src` and `dst` are aligned
// to their element and nothing more
template <typename T>
__device__ __forceinline__ void nearest_remap(const T *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1, const uint16_t *__restrict__ map2,
                                              int dw, int dh, T *__restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= dw) return;
    const size_t o = (size_t)y * dw + x;
    const T *s = src + (size_t)blockIdx.z * sw * sh;
    dst[(size_t)blockIdx.z * dw * dh + o] = (T)nearest_px<T>(s, sw, sh, map1[o * 2], map1[o * 2 + 1], map2[o] & (kQTab2 - 1));
}
__global__ void __launch_bounds__(256) k_remap_nn8(const uint8_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                  const uint16_t *__restrict__ map2, int dw, int dh, uint8_t *__restrict__ dst)
{
    nearest_remap<uint8_t>(src, sw, sh, map1, map2, dw, dh, dst);
}
__global__ void __launch_bounds__(256) k_remap_nn16(const uint16_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                   const uint16_t *__restrict__ map2, int dw, int dh, uint16_t *__restrict__ dst)
{
    nearest_remap<uint16_t>(src, sw, sh, map1, map2, dw, dh, dst);
}

}  // namespace bevw
