// Host-only check of the nearest-neighbour unit kernels (cameracalibration_amd/csrc: bevw_unit.h unit_gsrc_gray, bevw_kernels_nearest.h
// nearest_decode8 / nearest_decode16 / nearest_pack8 / nearest_pack16) -- runs without a GPU.  The plan compiler (unit_compile) makes the
// units of a caller's map as the library does for a one-camera plan; this program then walks k_units_nn8's and k_units_nn16's steps in
// program order, slot by slot, with the kernels' own __host__ __device__ functions:
//   * the group list is the one-channel list (unit_gsrc_gray), doubled at 16 bits where the kernel reads it; a slot without a group stays
//     the sentinel;
//   * every group slot is landed as ONE load of 8 bytes (8 bits) or 12 bytes (16 bits) at its offset in a frame set of fw * fh (* 2) bytes.
//     EVERY byte the load touches is held against the set's size: a dword wholly past the end reads as zero (the buffer descriptor's range
//     check) and is counted; the program FAILS on an offset that is not 4-byte aligned and on a dword that straddles the end.  8 bits: the
//     8 bytes land at 8 bytes per slot; 16 bits: {d0, d1} in plane 0 at 8 bytes per slot, d2 in plane 1 at 4 bytes per slot; a lane without
//     a group loads nothing (zeros);
//   * every lane decodes its entries to ONE LDS byte address per pixel, held against the unit's patch (inside it, aligned to the texel:
//     checked), reads its texel, masks its quad and stores it as 4 (8) bytes at a 4-byte (8-byte) multiple inside the image (checked), under
//     the kernel's store mask.
// tests/test_nearest_host.py compares what the units wrote with the NumPy statement of cv2's rule (tests/_nearest.py).
//
//   nearest_emulate <in> <out>
//   in : int32 fw fh bw bh nframes | int16 map1[bh][bw][2] | uint16 map2[bh][bw] | uint8 frames8[nframes][fh][fw] | uint16 frames16[nframes][fh][fw]
//   out: int32 nunits | uint8 written[bh][bw] (stores per pixel, both depths alike) | uint8 image8[nframes][bh][bw] | uint16 image16[nframes][bh][bw]
//        (unwritten pixels 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"
#include "../../cameracalibration_amd/csrc/bevw_kernels_nearest.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

struct Walk {
    int fw, fh, bw, bh, nframes, pitch;
    UnitPlanHost up;
    std::vector<uint32_t> gray;   // the one-channel group list
    size_t past_end = 0;
};

// one depth: bpp bytes per texel, frames = nframes frame sets, img = nframes images (zeroed), written = stores per pixel
static int walk(Walk &w, int bpp, const uint8_t *frames, uint8_t *img, std::vector<uint8_t> &written)
{
    const bool deep = bpp == 2;
    const size_t set_bytes = (size_t)w.fw * w.fh * bpp, img_bytes = (size_t)w.pitch * w.bh * bpp;
    CHECK(kPairNoGroup >= set_bytes, "the sentinel is inside the frame set");
    CHECK(2 * kNearestPatch8 <= 32768 && 2 * kNearestPatch16 <= 32768, "the block's LDS");
    const UnitPlanHost &up = w.up;
    for (int c = 0; c < kUnitClasses; ++c)
        for (uint32_t unit : up.list[c]) {
            const UnitDesc &d = up.desc[unit];
            const int NQ = kUnitClassNQ[c], GR = kUnitClassGR[c];
            const size_t plane0 = (size_t)GR * kUnitThreads * (deep ? kNearestPlane0Bytes16 : kNearestSlotBytes8);
            const size_t patch_bytes = plane0 + (deep ? (size_t)GR * kUnitThreads * kNearestPlane1Bytes16 : 0);
            CHECK(2 * patch_bytes <= 2 * (size_t)(deep ? kNearestPatch16 : kNearestPatch8), "patch");
            const int ux = (int)(int16_t)(d.pos & 0xffffu), uy = (int)(d.pos >> 16), uw = (int)(d.shape & 0xffffu), uh = (int)(d.shape >> 16);
            for (int b = 0; b < w.nframes; ++b) {
                const uint8_t *set = frames + (size_t)b * set_bytes;
                std::vector<uint8_t> patch(patch_bytes, 0xcd);
                if (d.groups != 0)
                    for (int r = 0; r < GR; ++r)
                        for (int tid = 0; tid < kUnitThreads; ++tid) {
                            const int slot = r * kUnitThreads + tid;
                            const uint32_t g = w.gray[((size_t)d.gs_off + r) * kUnitThreads + tid];
                            const uint32_t off = deep ? (g == kPairNoGroup ? kPairNoGroup : g * 2u) : g;
                            uint32_t v[3] = {0, 0, 0};   // a lane without a group is out of the descriptor's range: zeros
                            if (off != kPairNoGroup) {
                                CHECK(off % 4 == 0, "unit %u slot %d: offset %u is not 4-byte aligned", unit, slot, off);
                                CHECK((size_t)off + 4 * (size_t)bpp <= set_bytes, "unit %u slot %d: the group's own texels at %u leave the frames", unit, slot, off);
                                for (int k = 0; k < (deep ? 3 : 2); ++k) {
                                    const size_t o = (size_t)off + 4 * k;
                                    if (o + 4 <= set_bytes) memcpy(&v[k], set + o, 4);
                                    else { CHECK(o >= set_bytes, "unit %u slot %d: dword %d straddles the end of the frames", unit, slot, k); ++w.past_end; }
                                }
                            }
                            memcpy(patch.data() + (size_t)slot * 8, v, 8);
                            if (deep) memcpy(patch.data() + plane0 + (size_t)slot * kNearestPlane1Bytes16, &v[2], 4);
                        }
                for (int wave = 0; wave < kUnitWaves; ++wave)
                    for (int j = 0; j < NQ; ++j)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int sidx = unit_slot(wave, j);
                            int qx, row;
                            unit_quad(d.lq, sidx, lane, qx, row);
                            const uint32_t *e = up.entries.data() + (((size_t)d.ent_off + sidx) * 64 + lane) * 4;
                            const int x = ux + 4 * qx + unit_skew(up.skew, uy + row);
                            const bool store = 4 * qx < uw && row < uh && x >= 0 && x < w.pitch && !(unit_no_contributor(e[0]) && (e[0] & kUnitSkip));
                            uint32_t v[4] = {0, 0, 0, 0}, live[4] = {0, 0, 0, 0};
                            if (d.groups != 0)
                                for (int p = 0; p < 4; ++p) {
                                    const uint32_t a = deep ? nearest_decode16(e[p], (uint32_t)plane0) : nearest_decode8(e[p]);
                                    CHECK((a == kNearestNone) == unit_no_contributor(e[p]), "unit %u: entry %08x", unit, e[p]);
                                    if (a == kNearestNone) continue;   // (the kernel reads address 0 and masks the pixel)
                                    live[p] = 1;
                                    CHECK(a % (uint32_t)bpp == 0 && (size_t)a + bpp <= patch_bytes, "unit %u: entry %08x reads LDS byte %u outside the patch of %zu", unit, e[p], a, patch_bytes);
                                    if (deep) { uint16_t t; memcpy(&t, patch.data() + a, 2); v[p] = t; }
                                    else v[p] = patch[a];
                                }
                            if (!store) continue;
                            const size_t so = ((size_t)(uy + row) * w.pitch + (size_t)x) * bpp;
                            CHECK(so % (4 * (size_t)bpp) == 0 && so + 4 * (size_t)bpp <= img_bytes, "unit %u: quad store at %zu", unit, so);
                            if (deep) {
                                const uint2 q = nearest_pack16(v, make_uint2(live[0] * 0xffffu | live[1] * 0xffff0000u, live[2] * 0xffffu | live[3] * 0xffff0000u));
                                memcpy(img + (size_t)b * img_bytes + so, &q, 8);
                            } else {
                                const uint32_t q = nearest_pack8(v, live[0] * 0xffu | live[1] * 0xff00u | live[2] * 0xff0000u | live[3] * 0xff000000u);
                                memcpy(img + (size_t)b * img_bytes + so, &q, 4);
                            }
                            if (b == 0) for (int k = 0; k < 4; ++k) ++written[so / bpp + k];
                        }
            }
        }
    return 0;
}

static int run(int fw, int fh, int bw, int bh, int nframes, const std::vector<int16_t> &m1, const std::vector<uint16_t> &m2,
               const std::vector<uint8_t> &f8, const std::vector<uint16_t> &f16, const char *out_path)
{
    CHECK(fw % 4 == 0 && bw % 4 == 0, "the unit schedule serves source and destination widths that are multiples of 4");
    CHECK(fw <= 32768 && fh <= 32768, "a source beyond 32768 texels never takes the plan in nearest mode");
    const int tiles_x = (bw + 31) / 32, tiles_y = (bh + 7) / 8;
    std::vector<int16_t> l1[4] = {m1};
    std::vector<uint16_t> l2[4] = {m2};
    std::vector<uint8_t> mk[4] = {std::vector<uint8_t>((size_t)bw * bh, 255)};
    std::vector<uint32_t> hdr = unit_host_headers(l1, mk, 1, fw, fh, bw, bh, tiles_x, tiles_y);
    Walk w;
    w.fw = fw; w.fh = fh; w.bw = bw; w.bh = bh; w.nframes = nframes; w.pitch = bw;
    UnitTuning tune;
    tune.row_order = 4;   // as plan_build orders a one-camera plan
    unit_compile(l1, l2, mk, 1, fw, fh, bw, bh, w.pitch, tiles_x, tiles_y, hdr, w.up, tune);
    for (int c = 0; c < kUnitClasses; ++c) CHECK(kUnitClassCON[c] == 1 || w.up.list[c].empty(), "a one-camera plan with a two-contributor unit");
    unit_gsrc_gray(w.up.gsrc, fw, fh, w.gray);
    CHECK(w.gray.size() == w.up.gsrc.size(), "list size");
    std::vector<uint8_t> written8((size_t)bw * bh, 0), written16((size_t)bw * bh, 0), img8((size_t)nframes * bw * bh, 0);
    std::vector<uint16_t> img16((size_t)nframes * bw * bh, 0);
    if (walk(w, 1, f8.data(), img8.data(), written8)) return 1;
    if (walk(w, 2, reinterpret_cast<const uint8_t *>(f16.data()), reinterpret_cast<uint8_t *>(img16.data()), written16)) return 1;
    CHECK(written8 == written16, "the two depths store different pixels");
    printf("nearest units ok: %zu units, %zu slots, %zu dwords past the frames read as zero\n", w.up.desc.size(), w.gray.size(), w.past_end);
    FILE *f = fopen(out_path, "wb");
    CHECK(f, "cannot write %s", out_path);
    const int32_t head = (int32_t)w.up.desc.size();
    fwrite(&head, 4, 1, f);
    fwrite(written8.data(), 1, written8.size(), f);
    fwrite(img8.data(), 1, img8.size(), f);
    fwrite(img16.data(), 2, img16.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    if (argc != 3) { fprintf(stderr, "usage: nearest_emulate <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    CHECK(f, "cannot read %s", argv[1]);
    int32_t head[5];
    CHECK(fread(head, 4, 5, f) == 5, "short header");
    const int fw = head[0], fh = head[1], bw = head[2], bh = head[3], nframes = head[4];
    CHECK(fw > 0 && fh > 0 && bw > 0 && bh > 0 && nframes > 0, "bad header");
    const size_t npx = (size_t)bw * bh, ntex = (size_t)nframes * fw * fh;
    std::vector<int16_t> m1(npx * 2);
    std::vector<uint16_t> m2(npx), f16(ntex);
    std::vector<uint8_t> f8(ntex);
    CHECK(fread(m1.data(), 2, npx * 2, f) == npx * 2 && fread(m2.data(), 2, npx, f) == npx && fread(f8.data(), 1, ntex, f) == ntex &&
          fread(f16.data(), 2, ntex, f) == ntex, "short input");
    fclose(f);
    return run(fw, fh, bw, bh, nframes, m1, m2, f8, f16, argv[2]);
}
