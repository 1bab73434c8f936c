// bevw_kernels_gray_stitch.h -- the kernels of the four-camera stitch on one-channel frames (bevw_set_channels: BevGenerator on 8UC1 frames),
// under names of their own.  Included by bevwarp_gray_stitch.hip alone, behind bevw_plan.h with BEVW_PLAN_SHARED_ONLY and bevw_kernels_gray.h
// with BEVW_GRAY_SHARED_ONLY (and by tests/native/gray_stitch_emulate.cpp, which runs the __host__ __device__ functions below on a CPU).
//
// The plan is the three-channel handle's: the same unit partition, the same entries, the same launch order, the same base tiles left to the
// per-tap kernel.  A group slot holds what it holds for the one-channel remapper (bevw_kernels_gray.h): the 8 bytes at the group's offset in
// a frame set of 4 * FW * FH bytes, landed in LDS as fetched; gray_decode, gray_pixel and gray_pack are that header's, unchanged.  What the
// stitch adds is what a one-camera plan never has: the two-contributor unit classes (seams, blend overlaps) with their blend weights, the
// car sprite, masks in the per-tap kernel, and a per-pixel stitch.  Everything outside the balance chain is per channel in the reference --
// cv2.remap, bitwise_and with the mask (direct) or trunc(f32(v) * f32(m / 255.0)) (blend), cv2.add -- so a byte here is channel 0 of the
// three-channel stitch of the replicated frames.
#pragma once
#include "bevw_kernels_gray.h"

namespace bevw {

// the arguments of the unit kernel and of the per-tap kernel: the plan's, and the sprite's row pitch
struct GrayStitchArgs {
    PlanArgs p;        // p.pitch: bytes per row of p.out; p.car: the sprite, rows of car_pitch bytes, or nullptr
    int car_pitch;     // p.bw (the caller's dense sprite: p.bw % 4 == 0) or p.pitch (a copy at the images' pitch)
};

// cv2.add of the four bytes of two dwords: per-byte sums, saturated at 255
__host__ __device__ __forceinline__ uint32_t gray_add_sat4(uint32_t a, uint32_t b)
{
    const uint32_t lo = (a & 0x00ff00ffu) + (b & 0x00ff00ffu), hi = ((a >> 8) & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu);   // <= 510 per field
    const uint32_t sl = ((lo >> 8) & 0x00010001u) * 255u, sh = ((hi >> 8) & 0x00010001u) * 255u;                            // 255 where a field carried
    return ((lo | sl) & 0x00ff00ffu) | (((hi | sh) & 0x00ff00ffu) << 8);
}
// one pixel of a two-contributor unit from the accumulators of its contributors (gray_pixel's form: the byte in bits 16..23).  BLEND: each
// value times its weight, trunc(f32(v) * f32(m / 255.0)) in the exact integer form (blend_apply_q23; w = blend_weight_q23(m)); direct: the
// values themselves (a pixel inside a mask has weight 1, a pixel without the contributor interpolates to 0).  The sum saturates (cv2.add).
template <bool BLEND>
__host__ __device__ __forceinline__ uint32_t gray_stitch_px2(uint32_t acc0, uint32_t acc1, uint32_t w0, uint32_t w1)
{
    const uint32_t v0 = (acc0 >> 16) & 255u, v1 = (acc1 >> 16) & 255u;
    const uint32_t s = (BLEND ? blend_apply_q23(v0, w0) : v0) + (BLEND ? blend_apply_q23(v1, w1) : v1);
    return s < 255u ? s : 255u;
}
// the dword of a lane's quad: one contributor (every weight is 255: gray_pack as it is) or two
template <bool BLEND, int NCON>
__host__ __device__ __forceinline__ uint32_t gray_stitch_quad(const uint32_t acc[NCON][4], const uint32_t wq[NCON][4])
{
    if (NCON == 1) return gray_pack(acc[0]);
    uint32_t d = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) d |= gray_stitch_px2<BLEND>(acc[0][p], acc[NCON - 1][p], wq[0][p], wq[NCON - 1][p]) << (8 * p);
    return d;
}

// ---- the unit kernel ------------------------------------------------------------------------------------------------------------------
// The lane of mono_unit_run (bevw_mono_unit.h has the loop and the frame ring) for every class of the stitch.  The fetch and the landing
// are GrayLane's (bevw_kernels_gray.h): ONE 8-byte load per group slot through the frame set's range-checked descriptor (4 * FW * FH bytes;
// the plan hands no unit the one group whose load would reach past it), landed as fetched; both halves of the ring fit for every class,
// two-contributor ones included (GR <= 4: 8 KB per half).
// NCON == 2 (classes 4, 5, 6): the plan holds three uint4 per lane and quad slot -- the entries of contributor 0, of contributor 1, and the
// two u8 blend weights of every pixel (w0 | w1 << 8) -- read as plan_unit_run reads them.
// The car sprite: a quad's four bytes are one dword through a range-checked descriptor of its own (num_records 0 without a sprite: zeros, no
// memory touched), read ONCE per unit before the frame loop, kept in one register per quad slot and added with saturation per byte; a wave
// whose quads see only zeros skips the add.  A unit without groups (under the car) stores the sprite or zeros in whole row runs.
template <bool BLEND, int NQ, int GR, int NCON>
struct GrayStitchLane : GraySlots<GR> {
    static_assert(NCON == 1 || NCON == 2, "unit class");
    static constexpr int kNQ = NQ, kPart = NCON == 2 ? 3 : 1;   // (plan_unit_run's narrow part)
    static constexpr bool kWeights = BLEND && NCON == 2;
    typedef uint32_t Quad;
    const int car_pitch;                  // bytes per row of the sprite
    const __amdgpu_buffer_rsrc_t rcar;    // the sprite; num_records 0 without one
    uint32_t a0[NQ][NCON][4], a1[NQ][NCON][4], pk[NQ][NCON][4], wx[NQ][NCON][4], wy[NQ][NCON][4], wq[NQ][NCON][4], car[NQ];
    uint32_t car_or = 0;
    bool car_any = false;

    __device__ __forceinline__ GrayStitchLane(const PlanArgs &a, int pitch)
        : car_pitch(pitch), rcar(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.car != nullptr ? a.car : a.out), 0,
                                                                   a.car != nullptr ? (uint32_t)pitch * (uint32_t)a.bh : 0u, kBufferWord3)) {}

    __device__ __forceinline__ uint32_t load(int j, const uint4 *ent)
    {
        uint32_t e0 = 0;
#pragma unroll
        for (int con = 0; con < NCON; ++con) {
            const uint4 e4 = unit_plan_load(ent + con * 64);
            const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
            if (con == 0) e0 = e[0];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                gray_decode(e[p], a0[j][con][p], a1[j][con][p], pk[j][con][p], wx[j][con][p], wy[j][con][p]);
                wq[j][con][p] = 0u;
            }
        }
        if (kWeights) {
            const uint4 w4 = unit_plan_load(ent + 2 * 64);
            const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int p = 0; p < 4; ++p) { wq[j][0][p] = blend_weight_q23(w[p] & 255u); wq[j][NCON - 1][p] = blend_weight_q23((w[p] >> 8) & 255u); }
        }
        return e0;
    }
    // the sprite's dword under the quad; out of range of the sprite's buffer descriptor: not read
    __device__ __forceinline__ void place(int j, bool store, int x, int y)
    {
        const uint32_t coff = (store && x < car_pitch) ? (uint32_t)y * (uint32_t)car_pitch + (uint32_t)x : kPairNoGroup;
        car[j] = __builtin_amdgcn_raw_buffer_load_b32(rcar, (int)coff, 0, 0);
        car_or |= car[j];
    }
    __device__ __forceinline__ void ready() { car_any = __builtin_amdgcn_ballot_w64(car_or != 0) != 0; }
    __device__ __forceinline__ Quad empty(int j) const { return car[j]; }   // under the car: the sprite or zeros
    __device__ __forceinline__ Quad quad(int j, const uint8_t *pw) const
    {
        uint32_t acc[NCON][4];
#pragma unroll
        for (int con = 0; con < NCON; ++con)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                acc[con][p] = gray_pixel(*reinterpret_cast<const uint2 *>(pw + a0[j][con][p]), *reinterpret_cast<const uint2 *>(pw + a1[j][con][p]),
                                         pk[j][con][p], wx[j][con][p], wy[j][con][p]);
        const uint32_t d = gray_stitch_quad<BLEND, NCON>(acc, wq[j]);
        return car_any ? gray_add_sat4(d, car[j]) : d;   // uniform over the wave
    }
};

// a unit of class C through the shared loop
template <bool BLEND, int C>
__device__ __forceinline__ void gray_stitch_class(const GrayStitchArgs &g, uint32_t chunk, uint32_t unit, uint8_t *lds)
{
    GrayStitchLane<BLEND, kUnitClassNQ[C], kUnitClassGR[C], kUnitClassCON[C]> ln(g.p, g.car_pitch);
    mono_unit_run(g.p, ln, chunk, unit, lds);
}

// every unit of every class in the partition's own order, one launch per step: plan_unit_any's block map and class switch
template <bool BLEND>
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_stitch_units_gray(GrayStitchArgs g)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[2 * kGrayPatch];
    uint32_t chunk, group;
    if (!plan_block_map(g.p, blockIdx.x, chunk, group)) return;
    if ((int)group >= g.p.nlist) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(g.p.tile_list[group]), unit = e & 0x0fffffffu;
#define BEVW_GRAY_STITCH_CASE(C) case C: gray_stitch_class<BLEND, C>(g, chunk, unit, patch); break;
    switch (e >> 28) {
        BEVW_GRAY_STITCH_CASE(0) BEVW_GRAY_STITCH_CASE(1) BEVW_GRAY_STITCH_CASE(2) BEVW_GRAY_STITCH_CASE(3)
        BEVW_GRAY_STITCH_CASE(4) BEVW_GRAY_STITCH_CASE(5) BEVW_GRAY_STITCH_CASE(7)
        default: gray_stitch_class<BLEND, 6>(g, chunk, unit, patch); break;
    }
#undef BEVW_GRAY_STITCH_CASE
}

// ---- the per-tap tile kernel -----------------------------------------------------------------------------------------------------------
// k_stitch_plan's body on one channel: one wave per 32 x 8 base tile of the list (the tiles no unit owns: footprints on the frame border),
// lane l owns the pixel quad (l % 8, l / 8), every tap read straight from the frames (remap_u8c1_px: a tap outside the frame is 0).  The
// first and, where the tile's header says so, the second contributor of every pixel; BLEND: every value times the weight of its mask byte;
// saturating sums; a tile without any contributor (kHdrEmpty) has no valid entry and comes out as zeros; then the sprite; one dword store per
// lane through the image's range-checked descriptor.  Rows of a.pitch bytes, a.pitch % 4 == 0.
template <bool BLEND>
__global__ void __launch_bounds__(256) k_stitch_tiles_gray(GrayStitchArgs g)
{
    const PlanArgs &a = g.p;
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    const int lane = threadIdx.x & 63;
    const int slot = (int)group * (int)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (slot >= a.nlist) return;
    const int tile = a.tile_list ? (int)__builtin_amdgcn_readfirstlane(a.tile_list[slot]) : slot;
    const uint32_t hdr = __builtin_amdgcn_readfirstlane(a.hdr[tile]);
    const bool second = hdr & kHdrSecond;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x0 = (tx * kPlanLX + lane % kPlanLX) * 4, y = ty * kPlanLY + lane / kPlanLX;
    if (x0 >= a.bw || y >= a.bh) return;
    const size_t set_bytes = (size_t)a.fw * a.fh * a.ncams, img_bytes = (size_t)a.pitch * a.bh;
    EntryRegs e[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e[0][j] = decode_entry(a.plan[((size_t)tile * 8 + j) * 64 + lane], false);
        e[1][j] = decode_entry(second ? a.plan[((size_t)tile * 8 + 4 + j) * 64 + lane] : make_uint2(0, 0), false);
        entry_to_taps(e[0][j], a.fw, (uint32_t)a.fw * a.fh * 3);   // (the plan's interior entries hold BGR frame-set offsets)
        entry_to_taps(e[1][j], a.fw, (uint32_t)a.fw * a.fh * 3);
    }
    uint32_t car = 0;
    if (a.car != nullptr && x0 < g.car_pitch) car = *reinterpret_cast<const uint32_t *>(a.car + (size_t)y * g.car_pitch + x0);
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const uint8_t *fb = a.frames + (size_t)b * set_bytes;
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t s = 0;
#pragma unroll
            for (int con = 0; con < 2; ++con) {
                const EntryRegs &t = e[con][j];
                if (!(t.meta & kMetaValid)) continue;
                const int cam = (t.meta >> 18) & 3, sx = (int)(int16_t)(t.off & 0xffffu), sy = (int)(int16_t)(t.off >> 16);
                const uint32_t v = (uint32_t)remap_u8c1_px(fb + (size_t)cam * a.fw * a.fh, a.fw, a.fh, sx, sy, t.meta & 1023u, 0);
                s += BLEND ? blend_apply_q23(v, blend_weight_q23((t.meta >> 10) & 255u)) : v;
            }
            d |= (s < 255u ? s : 255u) << (8 * j);
        }
        d = gray_add_sat4(d, car);
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3);
        unit_store_dword(d, ro, (int)((uint32_t)y * (uint32_t)a.pitch + (uint32_t)x0), false);
    }
}

// ---- the per-pixel stitch ----------------------------------------------------------------------------------------------------------------
// k_stitch_pp on one channel: one thread per BEV pixel loops the four cameras through LUT and mask -- always valid (any width, any
// address, any number of contributors, both tie rules), byte loads and byte stores.  Images with rows of `pitch` bytes, the sprite dense.
// grid = (ceil(bw / 256), bh, frame sets)
template <bool BLEND>
__global__ void __launch_bounds__(256) k_stitch_pp_gray(const uint8_t *__restrict__ frames, int fw, int fh, StitchTables T, int bw, int bh,
                                                       const uint8_t *__restrict__ car, uint8_t *__restrict__ out, int pitch, int ties_even)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int b = blockIdx.z;
    if (x >= bw) return;
    const size_t o = (size_t)y * bw + x, frame_bytes = (size_t)fw * fh;
    uint32_t acc = 0;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        const uint32_t m = T.mask[c][o];
        if (m == 0) continue;
        const uint8_t *src = frames + ((size_t)b * 4 + c) * frame_bytes;
        const uint32_t v = (uint32_t)remap_u8c1_px(src, fw, fh, T.lut1[c][o * 2], T.lut1[c][o * 2 + 1], T.lut2[c][o] & (kQTab2 - 1), ties_even);
        acc = min(255u, acc + (BLEND ? blend_apply_q23(v, blend_weight_q23(m)) : v));
    }
    if (car != nullptr) acc = min(255u, acc + car[o]);
    out[((size_t)b * bh + y) * pitch + x] = (uint8_t)acc;
}

}  // namespace bevw
