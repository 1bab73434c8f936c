// bevw_mono_unit.h -- what the one-channel kernel families share: the unit loop (mono_unit_run), the per-tap tile walk (mono_tiles), the
// one-thread-per-pixel remap (mono_remap) and the two quad stores (mono_store).  No kernel lives here: bevw_kernels_gray.h,
// bevw_kernels_gray16.h, bevw_kernels_nearest.h and bevw_kernels_gray_stitch.h hold the kernels, under their own names and in their own
// translation units, and give these bodies what is theirs -- the texel, the LDS layout, the arithmetic.
#pragma once
#include "bevw_plan.h"

namespace bevw {

// a lane's quad to the image: 4 bytes (8-bit texels) or 8 (16-bit texels), streamed where the rows are whole sectors (unit_store_quad's rule)
__device__ __forceinline__ void mono_store(uint32_t v, __amdgpu_buffer_rsrc_t ro, int off, bool streaming) { unit_store_dword(v, ro, off, streaming); }
__device__ __forceinline__ void mono_store(uint2 v, __amdgpu_buffer_rsrc_t ro, int off, bool streaming)
{
    const pair_u32x2 d = {v.x, v.y};
    if (streaming) __builtin_amdgcn_raw_buffer_store_b64(d, ro, off, 0, kPairStreamAux);
    else __builtin_amdgcn_raw_buffer_store_b64(d, ro, off, 0, kPairStoreAux);
}

// ---- the unit loop ----------------------------------------------------------------------------------------------------------------------
// plan_unit_run (bevw_unit.h) for one channel: one block of 4 waves owns a unit for the frames of its batch chunk.  Per frame every lane
// fetches up to GR group slots -- ONE load each (Lane::fetch: 8 bytes at 1 byte per texel, 12 at 2) at the slot's 4-byte aligned offset
// (unit_gsrc_gray; Lane::group_offset doubles it at 2 bytes per texel) through the frame set's range-checked descriptor, as the NV12 unit
// kernel fetches its Y bytes.
// The end of the set.  Only the last group of the set's last row would reach a dword past the set (it would read as zero and touch nothing;
// bevw_kernels_gray16.h has why no dword of a 12-byte load straddles the end), and the plan never hands that group to a unit: unit_compile
// drops every base tile whose 16-byte BGR window would overrun the frame set, which is that group's (tests/test_gray_host.py holds it on a
// map that ends in the frame's last texel).  Texel 4g+4 of a row's last group is never sampled either (its footprint would cross the frame
// border: a base tile of the per-tap kernel).  A lane without a group is out of the descriptor's range as a whole, and so is the image
// offset of a quad that is not stored: an out-of-range lane touches nothing, and no branch guards it.
// The ring.  The groups of the next two frames are in flight in registers; Lane::land puts frame b+1 into the other half of the block's LDS
// while frame b is interpolated from this one (Lane::quad): one barrier per frame for every class, both halves fit (kPatch <= kMaxPatch).
// The loop takes two frames a turn, one per half; a chunk of odd length runs one frame past its end, where frame_of hands every load and
// every store the chunk's last frame once more: the same bytes written again.
//
// A lane is a struct over the unit class that keeps a lane's per-pixel registers across the frames:
//   kNQ, kGR                 the unit class: quad slots per lane, group slots per lane
//   kTexelBytes              bytes per source and destination texel
//   kPart                    uint4 per lane and quad slot in the entry list (1; 3 with two contributors and their weights)
//   kPatch, kMaxPatch        LDS bytes of one frame's patch for this class / for the largest class (the block's array holds two of those)
//   Quad, Fetch              a lane's stored quad (uint32_t or uint2: mono_store), a group slot as fetched
//   load(j, ent)             reads and decodes the entries of quad slot j; returns entry 0 of contributor 0 (the store predicate's)
//   place(j, store, x, y)    what else the slot needs from its place in the image (the stitch's sprite), ready() once after all slots
//   empty(j)                 the quad of a unit without groups
//   group_offset(g)          a group-list word -> the byte offset Lane::fetch loads
//   fetch(rs, off), land(half, idx, f), quad(j, patch)
template <class Lane>
__device__ __forceinline__ void mono_unit_run(const PlanArgs &a, Lane &ln, uint32_t chunk, uint32_t unit, uint8_t *lds)
{
    constexpr int NQ = Lane::kNQ, GR = Lane::kGR, kPatch = Lane::kPatch;
    constexpr uint32_t BPP = Lane::kTexelBytes;
    static_assert(NQ >= 1 && NQ <= kUnitMaxNQ && GR >= 1 && GR <= kUnitMaxGR, "unit class");
    static_assert(2 * kPatch <= 2 * Lane::kMaxPatch, "both halves of the frame ring fit the block's LDS");
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(a.un_desc + unit);
    const uint32_t pos = __builtin_amdgcn_readfirstlane(dp[0]), shape = __builtin_amdgcn_readfirstlane(dp[1]);
    const uint32_t ent_off = __builtin_amdgcn_readfirstlane(dp[2]), gs_off = __builtin_amdgcn_readfirstlane(dp[3]);
    const uint32_t lq = __builtin_amdgcn_readfirstlane(dp[4]);
    const uint32_t ngroups = __builtin_amdgcn_readfirstlane(dp[6]);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ux = (int)(int16_t)(pos & 0xffffu), uy = (int)(pos >> 16), uw = (int)(shape & 0xffffu), uh = (int)(shape >> 16);
    const size_t set_bytes = a.set_stride ? (size_t)a.set_stride : (size_t)a.fw * a.fh * a.ncams * BPP, img_bytes = (size_t)a.pitch * a.bh * BPP;
    const bool streaming = ((uint32_t)a.pitch * BPP) % 64u == 0u;   // rows of whole sectors (unit_store_quad's rule on bytes)

    uint32_t gs[GR], ooff[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int sidx = unit_slot(wave, j);
        int qx, row;
        unit_quad(lq, sidx, lane, qx, row);
        const int x = ux + 4 * qx + unit_skew((uint32_t)a.un_skew, uy + row);
        const uint32_t e0 = ln.load(j, a.un_entries + ((size_t)ent_off + sidx * Lane::kPart) * 64 + lane);   // the lane's 4 pixels of this slot
        const bool store = 4 * qx < uw && row < uh && x >= 0 && x < a.pitch && !(unit_no_contributor(e0) && (e0 & kUnitSkip));
        // out of range of the image's buffer descriptor: not written
        ooff[j] = store ? ((uint32_t)(uy + row) * (uint32_t)a.pitch + (uint32_t)x) * BPP : kPairNoGroup;
        ln.place(j, store, x, uy + row);
    }
    ln.ready();
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
    auto frame_of = [&](int b) { return min(b, b_end - 1); };   // past the chunk: the last frame once more
    auto image = [&](int b) { return __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)frame_of(b) * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3); };

    if (ngroups == 0) {
        // no contributor anywhere (the map leaves the frame; under the car): every frame of the chunk gets Lane::empty, in whole row runs
#pragma unroll 1
        for (int b = b_begin; b < b_end; ++b) {
            const __amdgpu_buffer_rsrc_t ro = image(b);
#pragma unroll
            for (int j = 0; j < NQ; ++j) mono_store(ln.empty(j), ro, (int)ooff[j], streaming);
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < GR; ++r) gs[r] = Lane::group_offset(once_load<BEVW_PLAN_NT>(a.un_gsrc + ((size_t)gs_off + r) * kUnitThreads + threadIdx.x));

    typename Lane::Fetch pf[2][GR];
    auto issue = [&](int b, int ring) {
        const uint8_t *src = a.frames + (size_t)frame_of(b) * set_bytes;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src), 0, (uint32_t)set_bytes, kBufferWord3);
#pragma unroll
        for (int r = 0; r < GR; ++r) pf[ring][r] = Lane::fetch(rs, (int)gs[r]);
    };
    auto land = [&](int ring) {   // the groups of ring slot `ring` -> the patch half of that frame
#pragma unroll
        for (int r = 0; r < GR; ++r) Lane::land(lds + ring * kPatch, r * kUnitThreads + (int)threadIdx.x, pf[ring][r]);
    };
    auto frame = [&](int b, int ring) {
        issue(b + 2, ring);        // the ring slot of frame b has landed
        typename Lane::Quad d[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) d[j] = ln.quad(j, lds + ring * kPatch);
        land(ring ^ 1);            // frame b+1 into the other half: nobody reads it before the barrier
        const __amdgpu_buffer_rsrc_t ro = image(b);   // past the chunk: re-writes the last frame with the same bytes
#pragma unroll
        for (int j = 0; j < NQ; ++j) mono_store(d[j], ro, (int)ooff[j], streaming);
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

// ---- the per-tap tile walk ----------------------------------------------------------------------------------------------------------------
// The base tiles no unit owns (footprints on the frame border): one wave per 32 x 8 base tile of the list, lane l owns the pixel quad
// (l % 8, l / 8), every tap read straight from the frame by px(src, sw, sh, sx, sy, code) -- the per-pixel function of the family, with its
// own range check.  k_stitch_plan's block map and entries; an entry without a contributor gives 0.  Rows of a.pitch == a.bw texels of T,
// a.bw % 4 == 0, a.out 4-byte aligned: one store per lane (mono_store).
// Used by k_tiles_nn8 / k_tiles_nn16.  k_stitch_plan_gray and k_stitch_plan_gray16 hold the same walk in their own text: they read the
// kernel's by-value arguments directly, and handing those to this body by reference alone gives them other machine code (another order of
// the scalar argument loads, other registers from there on), which a refactor of them must not.
template <typename T, class Px>
__device__ __forceinline__ void mono_tiles(const PlanArgs &a, Px px)
{
    constexpr uint32_t BPP = sizeof(T);
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
    const uint32_t off = ((uint32_t)y * (uint32_t)a.pitch + (uint32_t)x0) * BPP;
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const T *fb = reinterpret_cast<const T *>(a.frames) + (size_t)b * set_texels;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(e[j].meta & kMetaValid)) continue;
            const int cam = (e[j].meta >> 18) & 3, sx = (int)(int16_t)(e[j].off & 0xffffu), sy = (int)(int16_t)(e[j].off >> 16);
            v[j] = px(fb + (size_t)cam * a.fw * a.fh, a.fw, a.fh, sx, sy, e[j].meta & 1023u);
        }
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3);
        if constexpr (BPP == 2) mono_store(make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16)), ro, (int)off, false);
        else mono_store(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24), ro, (int)off, false);
    }
}

// ---- the per-pixel remap --------------------------------------------------------------------------------------------------------------------
// k_remap_lut on one-channel sources: one thread per destination pixel from map1 / map2 through the family's px; grid =
// (ceil(dw / 256), dh, images).  `src` and `dst` are aligned to their element and nothing more
template <typename T, class Px>
__device__ __forceinline__ void mono_remap(const T *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1, const uint16_t *__restrict__ map2,
                                           int dw, int dh, T *__restrict__ dst, Px px)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= dw) return;
    const size_t o = (size_t)y * dw + x;
    const T *s = src + (size_t)blockIdx.z * sw * sh;
    dst[(size_t)blockIdx.z * dw * dh + o] = (T)px(s, sw, sh, map1[o * 2], map1[o * 2 + 1], map2[o] & (kQTab2 - 1));
}

}  // namespace bevw
