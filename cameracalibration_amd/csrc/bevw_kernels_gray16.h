// bevw_kernels_gray16.h -- every kernel that reads 16-bit one-channel frames (bevw_remapper_set_depth: 16UC1 sources and destinations of a
// remapper), under names of their own.  Included by bevwarp_gray16.hip, behind bevw_plan.h with BEVW_PLAN_SHARED_ONLY (and by
// tests/native/gray16_emulate.cpp, which runs the __host__ __device__ functions below on a CPU).
//
// The plan is the one-channel remapper's: the same unit partition, the same entries (pair index, two group slots, fx, fy), the same launch
// order, and the SAME group list -- Plan::units[kLayoutGray] holds the byte offset of a group's first texel in a frame set of 1 byte per
// texel, and in 2 bytes per texel the group starts at exactly twice that (gray16_group_offset; the no-group sentinel stays what it is, out
// of every frame set's range).  No plan layout of its own.
//
// What differs is the texel and the arithmetic.  A group is texels 4g .. 4g+4 of one source row: 10 bytes at byte offset 8g of the frame
// set, fetched as ONE 12-byte load {d0, d1, d2} = texels 4g .. 4g+5.  cv2.remap interpolates CV_16U with float32 weights, a float32 sum from
// left to right, cvRound and saturation -- remap_f32_px<uint16_t, 1> (bevw_device.h) -- and not in the Q15 fixed point of CV_8U: a 16-bit tap
// times an 11-bit weight needs up to 27 bits, so the products round, and no integer form reproduces them.  Both tie rules of
// BEVW_COMPAT_REMAP belong to the fixed-point path; this one rounds to nearest even always.
//
// LDS.  Pair k of a group (texels 4g+k, 4g+k+1) is 4 bytes at byte 2k of the 12: pairs 0, 1 lie inside {d0, d1}, pairs 2, 3 inside {d1, d2},
// and no single 8-byte aligned window of the 12 bytes as fetched holds all four (pair 3 is bytes 6 .. 9).  So a slot lands as two 8-byte
// halves in two PLANES of the frame's patch: plane 0 holds {d0, d1} of every slot, plane 1 holds {d1, d2}, 8 bytes per slot each (16 bytes
// per slot: 16 KB per frame for a 1024-group unit, 32 KB for the two halves of the frame ring -- the three-channel kernel's budget).  A pixel
// reads ONE ds_read_b64 per footprint row at plane (k >> 1), slot s -- 8-byte aligned, the 64-bank form -- and shifts its pair down by
// 2 * (k & 1) bytes (v_alignbyte_b32).  Consecutive slots of one plane are 8 bytes apart, as in the 8-bit kernel: the 32 lanes of a read
// group that walk consecutive slots cover the 256-byte bank row once.  (One 16-byte slot per group read with ds_read_b64 at +0 / +8 would put
// lanes 16 slots apart on the same banks: 2-way for every smooth map; ds_read_b128 / ds_read_b96 of whole slots cost 4 / 8 LDS cycles per
// instruction against 2, and 4 / 3 registers per row.)
#pragma once
#include <cmath>

#include "bevw_plan.h"
#include "bevw_mono_unit.h"

namespace bevw {

constexpr int kGray16HalfBytes = 8;                                        // LDS bytes per group slot and plane
constexpr int kGray16Patch = 2 * kUnitMaxGroups * kGray16HalfBytes;        // the largest unit's patch of one frame (two planes); the block holds two

// the grey plan's group offset (1 byte per texel) -> the byte offset of the same group in 2 bytes per texel; a slot without a group stays
// out of range (twice the sentinel would wrap to 0)
__host__ __device__ __forceinline__ uint32_t gray16_group_offset(uint32_t g) { return g == kPairNoGroup ? kPairNoGroup : g * 2u; }

// one plan entry (unit_entry) -> the LDS byte offsets of its two slots inside a frame's patch (plane k >> 1 of `plane_bytes` each) and the
// byte shift of its pair, packed: a0 | shift | a1 << 16 (a0, a1 multiples of 8 below 2^14, shift 0 or 2); the four float weights
// ay*ax, ay*fx, fy*ax, fy*fx of remap_f32_px -- multiples of 1/1024 and exact -- or zeros for a pixel without a contributor (equal slots).
// A weight is n / 1024 with n <= 1024: 11 significant bits and an exponent >= -10, so binary16 holds it exactly, and the kernel keeps the
// four of a pixel as two packed pairs (gray16_weights_pack): half the registers for one v_cvt_f32_f16 per weight and frame.
typedef _Float16 gray16_h2 __attribute__((ext_vector_type(2)));
__host__ __device__ __forceinline__ void gray16_weights_pack(const float w[4], uint32_t &w01, uint32_t &w23)
{
    const gray16_h2 a = {(_Float16)w[0], (_Float16)w[1]}, b = {(_Float16)w[2], (_Float16)w[3]};
    w01 = __builtin_bit_cast(uint32_t, a);
    w23 = __builtin_bit_cast(uint32_t, b);
}
__host__ __device__ __forceinline__ void gray16_weights_unpack(uint32_t w01, uint32_t w23, float w[4])
{
    const gray16_h2 a = __builtin_bit_cast(gray16_h2, w01), b = __builtin_bit_cast(gray16_h2, w23);
    w[0] = (float)a.x; w[1] = (float)a.y; w[2] = (float)b.x; w[3] = (float)b.y;
}
__host__ __device__ __forceinline__ void gray16_decode(uint32_t e, uint32_t plane_bytes, uint32_t &aw, float w[4])
{
    const uint32_t k = e & 3u, s0 = (e >> 2) & 1023u, s1 = (e >> 12) & 1023u, fx = (e >> 22) & 31u, fy = e >> 27;
    const uint32_t base = (k >> 1) * plane_bytes;
    const uint32_t a0 = base + s0 * (uint32_t)kGray16HalfBytes, a1 = base + s1 * (uint32_t)kGray16HalfBytes;
    aw = a0 | (2u * (k & 1u)) | (a1 << 16);
    const uint32_t ax = 32u - fx, ay = 32u - fy;
    const float on = s0 != s1 ? 1.f / 1024 : 0.f;
    w[0] = (float)(ay * ax) * on; w[1] = (float)(ay * fx) * on; w[2] = (float)(fy * ax) * on; w[3] = (float)(fy * fx) * on;
}
__host__ __device__ __forceinline__ uint32_t gray16_addr0(uint32_t aw) { return aw & 0xfff8u; }
__host__ __device__ __forceinline__ uint32_t gray16_addr1(uint32_t aw) { return aw >> 16; }

// cvRound and saturate_cast<ushort>: rne_f and sat_u16 of bevw_device.h (device functions; the host twin serves the emulator alone)
__host__ __device__ __forceinline__ uint32_t gray16_round(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)sat_u16(rne_f(v));
#else
    const long r = lrintf(v);   // (round to nearest even: the default rounding mode)
    return (uint32_t)(r < 0 ? 0 : (r > 65535 ? 65535 : r));
#endif
}
// one pixel from the 8 bytes of its two slot halves: remap_f32_px's interior statement -- four taps converted to float, four products, three
// sums from left to right (no fused multiply-add: -ffp-contract=off), cvRound, saturation
__host__ __device__ __forceinline__ uint32_t gray16_pixel(uint2 q0, uint2 q1, uint32_t aw, const float w[4])
{
    const uint32_t sh = aw & 3u;
    const uint32_t t0 = px_alignbyte(q0.y, q0.x, sh), t1 = px_alignbyte(q1.y, q1.x, sh);   // the pair's two texels in the halves of a dword
    const float v = (float)(t0 & 0xffffu) * w[0] + (float)(t0 >> 16) * w[1] + (float)(t1 & 0xffffu) * w[2] + (float)(t1 >> 16) * w[3];
    return gray16_round(v);
}
// a lane's 4 pixels -> its 8 bytes
__host__ __device__ __forceinline__ uint2 gray16_pack(const uint32_t v[4]) { return make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16)); }

// ---- the unit kernel ------------------------------------------------------------------------------------------------------------------
// The lane of mono_unit_run (bevw_mono_unit.h has the loop and the frame ring) for 2-byte texels and float weights.  Per frame every lane
// fetches up to GR group slots -- ONE 12-byte load each at the slot's offset 8g (4-byte aligned: frame sets are, and 8g is) through the
// frame set's range-checked descriptor (num_records = the set's bytes).
// The end of the set.  The 12 bytes of group g are texels 4g .. 4g+5.  Rows are whole groups (fw % 4 == 0), so for every group but a row's
// last all 12 bytes lie in the group's own row; a row's last group reads 4 bytes of the next row (texels 4g+4, 4g+5: never sampled -- a
// footprint on texel 4g+4 of a row's last group crosses the frame border, which is a base tile of the per-tap kernel), and only the last
// group of the set's last row reaches past the set: its third dword starts exactly at the set's end (the set is a multiple of 8 bytes), so it
// is out of range as a whole, reads as zero and touches nothing -- no dword ever straddles the end.  The plan never hands that group to a
// unit either (tests/native/gray16_emulate.cpp checks every byte of every load against the set's size and counts the dwords past it: 0,
// also on a map that ends in the frame's last texel).
// Registers.  The groups of the next two frames are in flight (2 x GR x 3 dwords).  The four weights of a pixel stay in registers across the
// frames as two binary16 pairs (exact: gray16_weights_pack) -- 16 pixels x 3 registers for the four-quad classes.  As four floats (16 x 5)
// the kernel spilled 57 registers to scratch at the 168 of three waves per SIMD; rebuilding them from fx, fy would cost 8 more vector
// instructions per pixel and frame against the 4 conversions, in a kernel whose float arithmetic is its longest chain already.
// Single-contributor classes only, as k_units_gray.  A lane's quad is 8 bytes: one dwordx2 store per quad slot.
template <int NQ, int GR>
struct Gray16Lane {
    static constexpr int kNQ = NQ, kGR = GR, kTexelBytes = 2, kPart = 1;
    static constexpr int kPlane = GR * kUnitThreads * kGray16HalfBytes, kPatch = 2 * kPlane, kMaxPatch = kGray16Patch;
    static_assert(kPatch <= 65536, "16-bit patch offsets");
    typedef uint2 Quad;
    typedef pair_u32x3 Fetch;
    uint32_t aw[NQ][4], w01[NQ][4], w23[NQ][4];

    __device__ __forceinline__ uint32_t load(int j, const uint4 *ent)
    {
        const uint4 e4 = unit_plan_load(ent);
        const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float w[4];
            gray16_decode(e[p], (uint32_t)kPlane, aw[j][p], w);
            gray16_weights_pack(w, w01[j][p], w23[j][p]);
        }
        return e[0];
    }
    __device__ __forceinline__ void place(int, bool, int, int) {}
    __device__ __forceinline__ void ready() {}
    __device__ __forceinline__ Quad empty(int) const { return make_uint2(0u, 0u); }   // the map leaves the frame: zeros
    static __device__ __forceinline__ uint32_t group_offset(uint32_t g) { return gray16_group_offset(g); }
    static __device__ __forceinline__ Fetch fetch(__amdgpu_buffer_rsrc_t rs, int off) { return __builtin_amdgcn_raw_buffer_load_b96(rs, off, 0, kPairLoadAux); }
    static __device__ __forceinline__ void land(uint8_t *half, int idx, Fetch f)   // {d0, d1} to plane 0, {d1, d2} to plane 1
    {
        uint2 *const q = reinterpret_cast<uint2 *>(half) + idx;
        q[0] = make_uint2(f.x, f.y);
        q[kPlane / kGray16HalfBytes] = make_uint2(f.y, f.z);
    }
    __device__ __forceinline__ Quad quad(int j, const uint8_t *pw)
    {
        uint32_t v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float w[4];
            // (the packed pairs are opaque to the optimiser here: it would hoist the conversions out of the frame loop otherwise, and
            // keep the four floats of every pixel after all -- 57 registers in scratch)
            asm volatile("" : "+v"(w01[j][p]), "+v"(w23[j][p]));
            gray16_weights_unpack(w01[j][p], w23[j][p], w);
            v[p] = gray16_pixel(*reinterpret_cast<const uint2 *>(pw + gray16_addr0(aw[j][p])), *reinterpret_cast<const uint2 *>(pw + gray16_addr1(aw[j][p])),
                                aw[j][p], w);
        }
        return gray16_pack(v);
    }
};

// every unit of every class in the partition's own order, one launch per step: k_units_gray's block map and class switch
__global__ void __launch_bounds__(kUnitThreads) __attribute__((amdgpu_waves_per_eu(BEVW_PLAN_ALL_WAVES, BEVW_PLAN_ALL_WAVES))) k_units_gray16(PlanArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t patch[2 * kGray16Patch];
    uint32_t chunk, group;
    if (!plan_block_map(a, blockIdx.x, chunk, group)) return;
    if ((int)group >= a.nlist) return;
    const uint32_t e = __builtin_amdgcn_readfirstlane(a.tile_list[group]), unit = e & 0x0fffffffu;
#define BEVW_GRAY16_CASE(C) case C: { static_assert(kUnitClassCON[C] == 1, "one contributor per pixel"); Gray16Lane<kUnitClassNQ[C], kUnitClassGR[C]> ln; mono_unit_run(a, ln, chunk, unit, patch); } break;
    switch (e >> 28) {
        BEVW_GRAY16_CASE(0) BEVW_GRAY16_CASE(1) BEVW_GRAY16_CASE(2) BEVW_GRAY16_CASE(3) BEVW_GRAY16_CASE(7)
        default: break;   // (two-contributor classes: the host makes no one-channel list for a plan that has such units)
    }
#undef BEVW_GRAY16_CASE
}

// ---- the per-tap and per-pixel kernels ------------------------------------------------------------------------------------------------------
// cv2.remap 16UC1, INTER_LINEAR with float weights, BORDER_CONSTANT 0: remap_f32_px<uint16_t, 1> (bevw_device.h) and saturation, one
// statement for interior and border footprints
__device__ __forceinline__ uint32_t remap_u16c1_px(const uint16_t *__restrict__ src, int sw, int sh, int sx, int sy, unsigned code)
{
    int o[1];
    remap_f32_px<uint16_t, 1>(src, sw, sh, sx, sy, code, o);
    return (uint32_t)sat_u16(o[0]);
}

// The per-tap tile kernel on 16-bit one-channel frames: k_stitch_plan_gray's block map, entries and lane layout (one wave per 32 x 8 base
// tile of the list, lane l owns the pixel quad (l % 8, l / 8)), every tap read straight from the frame.  Rows of a.pitch == a.bw pixels,
// a.bw % 4 == 0, a.out 4-byte aligned: one dwordx2 store per lane.  (Its own text, as k_stitch_plan_gray's and for the same reason.)
__global__ void __launch_bounds__(256) k_stitch_plan_gray16(PlanArgs a)
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
    const size_t set_texels = (size_t)a.fw * a.fh * a.ncams, img_bytes = (size_t)a.pitch * a.bh * 2;
    EntryRegs e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e[j] = decode_entry(a.plan[((size_t)tile * 8 + j) * 64 + lane], false);
        entry_to_taps(e[j], a.fw, (uint32_t)a.fw * a.fh * 3);   // (the plan's interior entries hold BGR frame-set offsets)
    }
    const int b_begin = (int)chunk * a.nb, b_end = min(a.batch, b_begin + a.nb);
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const uint16_t *fb = reinterpret_cast<const uint16_t *>(a.frames) + (size_t)b * set_texels;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(e[j].meta & kMetaValid)) continue;
            const int cam = (e[j].meta >> 18) & 3, sx = (int)(int16_t)(e[j].off & 0xffffu), sy = (int)(int16_t)(e[j].off >> 16);
            v[j] = remap_u16c1_px(fb + (size_t)cam * a.fw * a.fh, a.fw, a.fh, sx, sy, e[j].meta & 1023u);
        }
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)b * img_bytes, 0, (uint32_t)img_bytes, kBufferWord3);
        mono_store(gray16_pack(v), ro, (int)(((uint32_t)y * (uint32_t)a.pitch + (uint32_t)x0) * 2u), false);
    }
}

// k_remap_lut on 16-bit one-channel sources (mono_remap).  `src` and `dst` are 2-byte aligned and nothing more
__global__ void __launch_bounds__(256) k_remap_lut_gray16(const uint16_t *__restrict__ src, int sw, int sh, const int16_t *__restrict__ map1,
                                                         const uint16_t *__restrict__ map2, int dw, int dh, uint16_t *__restrict__ dst)
{
    mono_remap<uint16_t>(src, sw, sh, map1, map2, dw, dh, dst,
                         [](const uint16_t *s, int w, int h, int sx, int sy, unsigned code) { return remap_u16c1_px(s, w, h, sx, sy, code); });
}

}  // namespace bevw
