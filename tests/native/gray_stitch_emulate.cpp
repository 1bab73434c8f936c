// Host-only check of the one-channel stitch's unit kernel (cameracalibration_amd/csrc: bevw_unit.h unit_gsrc_gray on a four-camera list,
// bevw_kernels_gray.h gray_decode / gray_pixel / gray_pack, bevw_kernels_gray_stitch.h gray_stitch_quad / gray_add_sat4) -- runs without a
// GPU.  The plan compiler (unit_compile) makes the units of a rig's tables and masks as the library does for a handle; this program then
// walks k_stitch_units_gray's steps in program order with the kernel's own __host__ __device__ functions:
//   * the group lists are translated by unit_gsrc_gray and every slot is held against o / 3 of its BGR offset o;
//   * every group slot is landed as ONE 8-byte load at its offset in a frame set of ncams * fw * fh bytes: a dword past the end of the set
//     reads as zero (the buffer descriptor's range check), a lane without a group loads nothing.  The program FAILS on an offset that is
//     not 4-byte aligned, on a dword that straddles the end of the set, and on a pixel whose used bytes lie past the set;
//   * every lane of every class the plan holds -- the two-contributor ones read three uint4 per quad slot: both contributors' entries and
//     the weight word -- decodes its entries, reads the 8 bytes of its slots from the patch (inside the unit's patch, 8-byte aligned:
//     checked), interpolates, applies the blend weights or the plain saturating sum, adds the car's dword and stores its quad as one dword
//     at a 4-byte aligned offset inside the image (checked), under the kernel's store mask; a unit without groups stores the car or zeros.
// It fails unless a two-contributor class is present, every quad of a claimed base tile is stored exactly once, and no quad of an
// unclaimed tile is touched.  tests/test_gray_stitch_host.py compares the bytes the units wrote with the specification.
//
//   gray_stitch_emulate <in> <out>
//   in : int32 fw fh bw bh ncams nframes has_car blend | per camera: int16 lut1[bh][bw][2], uint16 lut2[bh][bw], uint8 mask[bh][bw]
//        | uint8 frames[nframes][ncams][fh][fw] | uint8 car[bh][bw] if has_car
//   out: int32 nunits claimed_tiles two_contributor_units classes_present (bit c: class c) | uint8 written[bh][bw] (stores per byte)
//        | uint8 image[nframes][bh][bw] (unwritten pixels 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"
#include "../../cameracalibration_amd/csrc/bevw_kernels_gray_stitch.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

struct Rig {
    int fw, fh, bw, bh, ncams, nframes, has_car, blend;
    std::vector<int16_t> l1[4];
    std::vector<uint16_t> l2[4];
    std::vector<uint8_t> mk[4];
    std::vector<uint8_t> frames, car;
};

// the quad of one lane from the accumulators of its contributors: the kernel's instantiation for (blend, NCON)
static uint32_t quad_of(bool blend, int ncon, const uint32_t acc[2][4], const uint32_t wq[2][4])
{
    if (ncon == 1) {
        const uint32_t a1[1][4] = {{acc[0][0], acc[0][1], acc[0][2], acc[0][3]}}, w1[1][4] = {{0, 0, 0, 0}};
        return blend ? gray_stitch_quad<true, 1>(a1, w1) : gray_stitch_quad<false, 1>(a1, w1);
    }
    return blend ? gray_stitch_quad<true, 2>(acc, wq) : gray_stitch_quad<false, 2>(acc, wq);
}

static int run(const Rig &r, const char *out_path)
{
    const int fw = r.fw, fh = r.fh, bw = r.bw, bh = r.bh;
    CHECK(fw % 4 == 0 && bw % 4 == 0, "the unit schedule serves frame widths and dense rows that are multiples of 4");
    const int tiles_x = (bw + 31) / 32, tiles_y = (bh + 7) / 8, pitch = bw;
    std::vector<uint32_t> hdr = unit_host_headers(r.l1, r.mk, r.ncams, fw, fh, bw, bh, tiles_x, tiles_y);
    UnitPlanHost up;
    unit_compile(r.l1, r.l2, r.mk, r.ncams, fw, fh, bw, bh, pitch, tiles_x, tiles_y, hdr, up, UnitTuning());
    CHECK(!up.desc.empty(), "no unit compiled");
    // ---- the list translation ----
    std::vector<uint32_t> gsrc;
    unit_gsrc_gray(up.gsrc, fw, fh, gsrc);
    CHECK(gsrc.size() == up.gsrc.size(), "list size");
    for (size_t i = 0; i < gsrc.size(); ++i) {
        if (up.gsrc[i] == kPairNoGroup) { CHECK(gsrc[i] == kPairNoGroup, "slot %zu: no group became %u", i, gsrc[i]); continue; }
        CHECK(up.gsrc[i] % 12 == 0 && gsrc[i] == up.gsrc[i] / 3, "slot %zu: BGR offset %u became %u", i, up.gsrc[i], gsrc[i]);
    }
    const size_t set_bytes = (size_t)fw * fh * r.ncams, img_bytes = (size_t)pitch * bh;
    std::vector<uint8_t> written((size_t)bw * bh, 0), img((size_t)r.nframes * img_bytes, 0);
    size_t past_end = 0, two = 0;
    uint32_t present = 0;
    for (int c = 0; c < kUnitClasses; ++c)
        for (uint32_t unit : up.list[c]) {
            const UnitDesc &d = up.desc[unit];
            const int NQ = kUnitClassNQ[c], GR = kUnitClassGR[c], NCON = kUnitClassCON[c], fpart = NCON == 2 ? 3 : 1;
            present |= 1u << c;
            two += NCON == 2;
            const size_t patch_bytes = (size_t)GR * kUnitThreads * kGraySlotBytes;
            CHECK(2 * patch_bytes <= 2 * (size_t)kGrayPatch, "patch");
            const int ux = (int)(int16_t)(d.pos & 0xffffu), uy = (int)(d.pos >> 16), uw = (int)(d.shape & 0xffffu), uh = (int)(d.shape >> 16);
            for (int b = 0; b < r.nframes; ++b) {
                const uint8_t *set = r.frames.data() + (size_t)b * set_bytes;
                std::vector<uint8_t> patch(patch_bytes, 0xcd);
                std::vector<uint32_t> slot_off((size_t)GR * kUnitThreads, kPairNoGroup);
                if (d.groups != 0)
                    for (int rr = 0; rr < GR; ++rr)
                        for (int tid = 0; tid < kUnitThreads; ++tid) {
                            const uint32_t off = gsrc[((size_t)d.gs_off + rr) * kUnitThreads + tid];
                            uint32_t w[2] = {0, 0};   // a lane without a group is out of the descriptor's range: zeros
                            if (off != kPairNoGroup) {
                                CHECK(off % 4 == 0, "unit %u slot %d: offset %u is not 4-byte aligned", unit, rr * kUnitThreads + tid, off);
                                for (int k = 0; k < 2; ++k) {
                                    const size_t o = (size_t)off + 4 * k;
                                    if (o + 4 <= set_bytes) memcpy(&w[k], set + o, 4);
                                    else { CHECK(o >= set_bytes, "unit %u slot %d: dword %d straddles the end of the frames", unit, rr * kUnitThreads + tid, k); ++past_end; }
                                }
                            }
                            slot_off[(size_t)rr * kUnitThreads + tid] = off;
                            memcpy(patch.data() + (size_t)(rr * kUnitThreads + tid) * kGraySlotBytes, w, 8);
                        }
                for (int wave = 0; wave < kUnitWaves; ++wave)
                    for (int j = 0; j < NQ; ++j)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int sidx = unit_slot(wave, j);
                            int qx, row;
                            unit_quad(d.lq, sidx, lane, qx, row);
                            const uint32_t *e = up.entries.data() + (((size_t)d.ent_off + (size_t)sidx * fpart) * 64 + lane) * 4;   // part k at e + k * 256
                            const int x = ux + 4 * qx + unit_skew(up.skew, uy + row);
                            const bool store = 4 * qx < uw && row < uh && x >= 0 && x < pitch && !(unit_no_contributor(e[0]) && (e[0] & kUnitSkip));
                            uint32_t acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, wq[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                            if (d.groups != 0)
                                for (int con = 0; con < NCON; ++con)
                                    for (int p = 0; p < 4; ++p) {
                                        uint32_t a0, a1, k, wx, wy;
                                        gray_decode(e[con * 256 + p], a0, a1, k, wx, wy);
                                        CHECK(a0 % 8 == 0 && a1 % 8 == 0 && (size_t)a0 + 8 <= patch_bytes && (size_t)a1 + 8 <= patch_bytes && k < 4,
                                              "unit %u: entry %08x reads outside the patch", unit, e[con * 256 + p]);
                                        if (wx != 0)   // a contributor: texels k, k + 1 of both slots are frame bytes
                                            for (uint32_t s : {a0 / 8u, a1 / 8u})
                                                CHECK(slot_off[s] != kPairNoGroup && (size_t)slot_off[s] + k + 1 < set_bytes,
                                                      "unit %u: entry %08x uses a byte past the frames (slot %u at %u)", unit, e[con * 256 + p], s, slot_off[s]);
                                        uint2 q0, q1;
                                        memcpy(&q0, patch.data() + a0, 8);
                                        memcpy(&q1, patch.data() + a1, 8);
                                        acc[con][p] = gray_pixel(q0, q1, k, wx, wy);
                                        if (NCON == 2 && r.blend) wq[con][p] = blend_weight_q23((e[2 * 256 + p] >> (8 * con)) & 255u);
                                    }
                            if (!store) continue;
                            const size_t so = (size_t)(uy + row) * pitch + (size_t)x;
                            CHECK(so % 4 == 0 && so + 4 <= img_bytes, "unit %u: quad store at %zu", unit, so);
                            uint32_t dq = d.groups != 0 ? quad_of(r.blend != 0, NCON, acc, wq) : 0u;
                            if (r.has_car) {
                                uint32_t cw;
                                memcpy(&cw, r.car.data() + (size_t)(uy + row) * bw + x, 4);   // (dense sprite: bw % 4 == 0)
                                dq = gray_add_sat4(dq, cw);
                            }
                            memcpy(img.data() + (size_t)b * img_bytes + so, &dq, 4);
                            if (b == 0) for (int k = 0; k < 4; ++k) ++written[so + k];
                        }
            }
        }
    CHECK(two > 0, "no two-contributor unit: classes 4, 5, 6 are what this check is about");
    for (int y = 0; y < bh; ++y)
        for (int x = 0; x < bw; ++x) {
            const bool claimed = hdr[(size_t)(y / 8) * tiles_x + x / 32] & kHdrBlock;
            CHECK(written[(size_t)y * bw + x] == (claimed ? 1 : 0), "pixel (%d, %d) of %s base tile: stored %d times", x, y, claimed ? "a claimed" : "an unclaimed",
                  written[(size_t)y * bw + x]);
        }
    printf("gray stitch units ok: %zu units (%zu with two contributors, classes %02x), %zu claimed tiles, %zu dwords past the frames read as zero\n",
           up.desc.size(), two, present, up.claimed_tiles, past_end);
    FILE *f = fopen(out_path, "wb");
    CHECK(f, "cannot write %s", out_path);
    const int32_t head[4] = {(int32_t)up.desc.size(), (int32_t)up.claimed_tiles, (int32_t)two, (int32_t)present};
    fwrite(head, 4, 4, f);
    fwrite(written.data(), 1, written.size(), f);
    fwrite(img.data(), 1, img.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    if (argc != 3) { fprintf(stderr, "usage: gray_stitch_emulate <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    CHECK(f, "cannot read %s", argv[1]);
    int32_t head[8];
    CHECK(fread(head, 4, 8, f) == 8, "short header");
    Rig r;
    r.fw = head[0]; r.fh = head[1]; r.bw = head[2]; r.bh = head[3]; r.ncams = head[4]; r.nframes = head[5]; r.has_car = head[6]; r.blend = head[7];
    CHECK(r.fw > 0 && r.fh > 0 && r.bw > 0 && r.bh > 0 && r.ncams >= 1 && r.ncams <= 4 && r.nframes > 0, "bad header");
    const size_t npx = (size_t)r.bw * r.bh;
    for (int c = 0; c < r.ncams; ++c) {
        r.l1[c].resize(npx * 2); r.l2[c].resize(npx); r.mk[c].resize(npx);
        CHECK(fread(r.l1[c].data(), 2, npx * 2, f) == npx * 2 && fread(r.l2[c].data(), 2, npx, f) == npx && fread(r.mk[c].data(), 1, npx, f) == npx, "short tables");
    }
    r.frames.resize((size_t)r.nframes * r.ncams * r.fw * r.fh);
    CHECK(fread(r.frames.data(), 1, r.frames.size(), f) == r.frames.size(), "short frames");
    if (r.has_car) {
        r.car.resize(npx);
        CHECK(fread(r.car.data(), 1, npx, f) == npx, "short car");
    }
    fclose(f);
    return run(r, argv[2]);
}
