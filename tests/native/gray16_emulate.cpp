// Host-only check of the 16-bit one-channel unit kernel (cameracalibration_amd/csrc: bevw_unit.h unit_gsrc_gray, bevw_kernels_gray16.h
// gray16_group_offset / gray16_decode / gray16_weights_pack / gray16_pixel / gray16_pack) -- runs without a GPU.  The plan compiler
// (unit_compile) makes the units of a caller's map as the library does for a one-camera plan; this program then walks k_units_gray16's steps
// in program order with the kernel's own __host__ __device__ functions:
//   * the group list is the 8-bit one-channel list (unit_gsrc_gray), doubled by gray16_group_offset; every slot is held against 2 * (o / 3) of
//     its BGR offset o, and a slot without a group stays the sentinel;
//   * every group slot is landed as ONE 12-byte load at its offset in a frame set of fw * fh * 2 bytes.  EVERY byte the load touches is held
//     against the set's size: a dword wholly past the end reads as zero (the buffer descriptor's range check) and is counted; the program
//     FAILS on an offset that is not 4-byte aligned and on a dword that straddles the end.  The 12 bytes land as {d0, d1} in plane 0 and
//     {d1, d2} in plane 1 of the patch, 8 bytes per slot and plane; a lane without a group loads nothing (zeros);
//   * every lane decodes its entries, packs and unpacks the weights as the kernel keeps them, reads the 8 bytes of its two slot halves from
//     the patch (inside the unit's patch, 8-byte aligned: checked), interpolates and stores its quad as 8 bytes at an 8-byte multiple inside
//     the image (checked), under the kernel's store mask.
// tests/test_gray16_host.py compares the uint16 the units wrote with oracle.remap on the uint16 array.
//
//   gray16_emulate <in> <out>
//   in : int32 fw fh bw bh nframes | int16 map1[bh][bw][2] | uint16 map2[bh][bw] | uint16 frames[nframes][fh][fw]
//   out: int32 nunits | uint8 written[bh][bw] (stores per pixel) | uint16 image[nframes][bh][bw] (unwritten pixels 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"
#include "../../cameracalibration_amd/csrc/bevw_kernels_gray16.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static int run(int fw, int fh, int bw, int bh, int nframes, const std::vector<int16_t> &m1, const std::vector<uint16_t> &m2,
               const std::vector<uint16_t> &frames, const char *out_path)
{
    CHECK(fw % 4 == 0 && bw % 4 == 0, "the unit schedule serves source and destination widths that are multiples of 4");
    const int tiles_x = (bw + 31) / 32, tiles_y = (bh + 7) / 8, pitch = bw;
    std::vector<int16_t> l1[4] = {m1};
    std::vector<uint16_t> l2[4] = {m2};
    std::vector<uint8_t> mk[4] = {std::vector<uint8_t>((size_t)bw * bh, 255)};
    std::vector<uint32_t> hdr = unit_host_headers(l1, mk, 1, fw, fh, bw, bh, tiles_x, tiles_y);
    UnitPlanHost up;
    UnitTuning tune;
    tune.row_order = 4;   // as plan_build orders a one-camera plan
    unit_compile(l1, l2, mk, 1, fw, fh, bw, bh, pitch, tiles_x, tiles_y, hdr, up, tune);
    std::vector<uint8_t> written((size_t)bw * bh, 0);
    std::vector<uint16_t> img((size_t)nframes * bw * bh, 0);
    for (int c = 0; c < kUnitClasses; ++c) CHECK(kUnitClassCON[c] == 1 || up.list[c].empty(), "a one-camera plan with a two-contributor unit");
    // ---- the list: the 8-bit one-channel translation, doubled where the kernel reads it ----
    std::vector<uint32_t> gray, gsrc;
    unit_gsrc_gray(up.gsrc, fw, fh, gray);
    CHECK(gray.size() == up.gsrc.size(), "list size");
    gsrc.resize(gray.size());
    for (size_t i = 0; i < gray.size(); ++i) {
        gsrc[i] = gray16_group_offset(gray[i]);
        if (up.gsrc[i] == kPairNoGroup) { CHECK(gsrc[i] == kPairNoGroup, "slot %zu: no group became %u", i, gsrc[i]); continue; }
        CHECK(up.gsrc[i] % 12 == 0 && gsrc[i] == up.gsrc[i] / 3 * 2 && gsrc[i] % 8 == 0, "slot %zu: BGR offset %u became %u", i, up.gsrc[i], gsrc[i]);
    }
    const size_t set_bytes = (size_t)fw * fh * 2, img_bytes = (size_t)pitch * bh * 2;
    CHECK(kPairNoGroup >= set_bytes, "the sentinel is inside the frame set");
    size_t past_end = 0, next_row = 0;
    for (int c = 0; c < kUnitClasses; ++c)
        for (uint32_t unit : up.list[c]) {
            const UnitDesc &d = up.desc[unit];
            const int NQ = kUnitClassNQ[c], GR = kUnitClassGR[c];
            const size_t plane_bytes = (size_t)GR * kUnitThreads * kGray16HalfBytes, patch_bytes = 2 * plane_bytes;
            CHECK(2 * patch_bytes <= 2 * (size_t)kGray16Patch && 2 * (size_t)kGray16Patch <= 32768, "patch");
            const int ux = (int)(int16_t)(d.pos & 0xffffu), uy = (int)(d.pos >> 16), uw = (int)(d.shape & 0xffffu), uh = (int)(d.shape >> 16);
            for (int b = 0; b < nframes; ++b) {
                const uint8_t *set = reinterpret_cast<const uint8_t *>(frames.data()) + (size_t)b * set_bytes;
                std::vector<uint8_t> patch(patch_bytes, 0xcd);
                if (d.groups != 0)
                    for (int r = 0; r < GR; ++r)
                        for (int tid = 0; tid < kUnitThreads; ++tid) {
                            const int slot = r * kUnitThreads + tid;
                            const uint32_t off = gsrc[((size_t)d.gs_off + r) * kUnitThreads + tid];
                            uint32_t w[3] = {0, 0, 0};   // a lane without a group is out of the descriptor's range: zeros
                            if (off != kPairNoGroup) {
                                CHECK(off % 4 == 0, "unit %u slot %d: offset %u is not 4-byte aligned", unit, slot, off);
                                CHECK((size_t)off + 8 <= set_bytes, "unit %u slot %d: the group's own texels at %u leave the frames", unit, slot, off);
                                for (int k = 0; k < 3; ++k) {
                                    const size_t o = (size_t)off + 4 * k;
                                    if (o + 4 <= set_bytes) memcpy(&w[k], set + o, 4);
                                    else { CHECK(o >= set_bytes, "unit %u slot %d: dword %d straddles the end of the frames", unit, slot, k); ++past_end; }
                                }
                                if (b == 0 && (off / 2 % (uint32_t)fw) + 4 == (uint32_t)fw) ++next_row;   // (a row's last group: its third dword is the next row's)
                            }
                            const uint32_t lo[2] = {w[0], w[1]}, hi[2] = {w[1], w[2]};
                            memcpy(patch.data() + (size_t)slot * kGray16HalfBytes, lo, 8);
                            memcpy(patch.data() + plane_bytes + (size_t)slot * kGray16HalfBytes, hi, 8);
                        }
                for (int wave = 0; wave < kUnitWaves; ++wave)
                    for (int j = 0; j < NQ; ++j)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int sidx = unit_slot(wave, j);
                            int qx, row;
                            unit_quad(d.lq, sidx, lane, qx, row);
                            const uint32_t *e = up.entries.data() + (((size_t)d.ent_off + sidx) * 64 + lane) * 4;
                            const int x = ux + 4 * qx + unit_skew(up.skew, uy + row);
                            const bool store = 4 * qx < uw && row < uh && x >= 0 && x < pitch && !(unit_no_contributor(e[0]) && (e[0] & kUnitSkip));
                            uint32_t v[4] = {0, 0, 0, 0};
                            if (d.groups != 0)
                                for (int p = 0; p < 4; ++p) {
                                    uint32_t aw, w01, w23;
                                    float w[4], wk[4];
                                    gray16_decode(e[p], (uint32_t)plane_bytes, aw, w);
                                    gray16_weights_pack(w, w01, w23);
                                    gray16_weights_unpack(w01, w23, wk);
                                    CHECK(memcmp(w, wk, sizeof w) == 0, "unit %u: entry %08x: a weight is not exact in binary16", unit, e[p]);
                                    const uint32_t a0 = gray16_addr0(aw), a1 = gray16_addr1(aw);
                                    CHECK(a0 % 8 == 0 && a1 % 8 == 0 && (size_t)a0 + 8 <= patch_bytes && (size_t)a1 + 8 <= patch_bytes && (aw & 3u) % 2 == 0,
                                          "unit %u: entry %08x reads outside the patch", unit, e[p]);
                                    uint2 q0, q1;
                                    memcpy(&q0, patch.data() + a0, 8);
                                    memcpy(&q1, patch.data() + a1, 8);
                                    v[p] = gray16_pixel(q0, q1, aw, wk);
                                }
                            if (!store) continue;
                            const size_t so = ((size_t)(uy + row) * pitch + (size_t)x) * 2;
                            CHECK(so % 8 == 0 && so + 8 <= img_bytes, "unit %u: quad store at %zu", unit, so);
                            const uint2 dq = gray16_pack(v);
                            memcpy(reinterpret_cast<uint8_t *>(img.data()) + (size_t)b * img_bytes + so, &dq, 8);
                            if (b == 0) for (int k = 0; k < 4; ++k) ++written[so / 2 + k];
                        }
            }
        }
    printf("gray16 units ok: %zu units, %zu slots, %zu dwords past the frames read as zero, %zu groups end a row\n", up.desc.size(), gsrc.size(), past_end, next_row);
    FILE *f = fopen(out_path, "wb");
    CHECK(f, "cannot write %s", out_path);
    const int32_t head = (int32_t)up.desc.size();
    fwrite(&head, 4, 1, f);
    fwrite(written.data(), 1, written.size(), f);
    fwrite(img.data(), 2, img.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    if (argc != 3) { fprintf(stderr, "usage: gray16_emulate <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    CHECK(f, "cannot read %s", argv[1]);
    int32_t head[5];
    CHECK(fread(head, 4, 5, f) == 5, "short header");
    const int fw = head[0], fh = head[1], bw = head[2], bh = head[3], nframes = head[4];
    CHECK(fw > 0 && fh > 0 && bw > 0 && bh > 0 && nframes > 0, "bad header");
    const size_t npx = (size_t)bw * bh;
    std::vector<int16_t> m1(npx * 2);
    std::vector<uint16_t> m2(npx);
    std::vector<uint16_t> frames((size_t)nframes * fw * fh);
    CHECK(fread(m1.data(), 2, npx * 2, f) == npx * 2 && fread(m2.data(), 2, npx, f) == npx && fread(frames.data(), 2, frames.size(), f) == frames.size(), "short input");
    fclose(f);
    return run(fw, fh, bw, bh, nframes, m1, m2, frames, argv[2]);
}
