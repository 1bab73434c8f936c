// Host-only check of the NV12 store stage of the unit kernel (cameracalibration_amd/csrc/bevw_unit.h: plan_unit_run<.., OUT_NV12>) -- runs
// without a GPU.  The plan compiler (unit_compile) builds the units of real tables, and unit_emulate runs every unit on every frame with the
// NV12 store stage (UnitNv12Out: nv12_quad and the Y / U / V offsets of bevw_device.h, as the kernel stores them).  tests/test_nv12_out_host.py
// compares the result with the NumPy specification (tests/_nv12_out_spec.py) applied to the oracle's BGR output, and checks that every Y byte
// and every U / V pair of the units' area is stored exactly once.  Also checked here: every unit quad starts at a column x % 4 == 0.
//
//   nv12_out_emulate <in> <out> <pitch>
//   in : the input file of tests/native/unit_emulate.cpp (int32 fw fh bw bh ncams nframes has_car blend | tables | frames | car)
//   out: int32 nunits claimed_tiles | uint8 claimed[bh][pitch] (pixels of unit-owned base tiles, padding columns included)
//        | uint8 y_written[bh][pitch] | uint8 uv_written[bh / 2][pitch / 2] | uint8 image[nframes][bh * 3 / 2][pitch] (unwritten bytes 0)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    CHECK(argc == 4, "usage: nv12_out_emulate <in> <out> <pitch>");
    FILE *f = fopen(argv[1], "rb");
    CHECK(f, "cannot read %s", argv[1]);
    int32_t head[8];
    CHECK(fread(head, 4, 8, f) == 8, "short header");
    const int fw = head[0], fh = head[1], bw = head[2], bh = head[3], ncams = head[4], nframes = head[5], has_car = head[6], blend = head[7] & 1;
    const int pitch = atoi(argv[3]);
    CHECK(bw % 4 == 0 && bw % 2 == 0 && bh % 2 == 0 && pitch >= bw && pitch % 4 == 0, "geometry %d x %d, pitch %d", bw, bh, pitch);
    const size_t npx = (size_t)bw * bh;
    std::vector<int16_t> l1[4];
    std::vector<uint16_t> l2[4];
    std::vector<uint8_t> mk[4];
    for (int c = 0; c < ncams; ++c) {
        l1[c].resize(npx * 2); l2[c].resize(npx); mk[c].resize(npx);
        CHECK(fread(l1[c].data(), 2, npx * 2, f) == npx * 2 && fread(l2[c].data(), 2, npx, f) == npx && fread(mk[c].data(), 1, npx, f) == npx, "short tables");
    }
    const size_t set_bytes = (size_t)fw * fh * 3 * ncams;
    std::vector<uint8_t> frames((size_t)nframes * set_bytes), car, car_p;
    CHECK(fread(frames.data(), 1, frames.size(), f) == frames.size(), "short frames");
    if (has_car) {
        car.resize(npx * 3);
        CHECK(fread(car.data(), 1, car.size(), f) == car.size(), "short car");
        car_p.assign((size_t)pitch * bh * 3, 0);   // the sprite with rows of `pitch` pixels, as plan_stitch pads it
        for (int y = 0; y < bh; ++y) memcpy(car_p.data() + (size_t)y * pitch * 3, car.data() + (size_t)y * bw * 3, (size_t)bw * 3);
    }
    fclose(f);

    const int tiles_x = (bw + 31) / 32, tiles_y = (bh + 7) / 8;
    std::vector<uint32_t> hdr = unit_host_headers(l1, mk, ncams, fw, fh, bw, bh, tiles_x, tiles_y);
    UnitPlanHost up;
    UnitTuning tune;
    tune.wide_double = 1;   // as plan_build
    unit_compile(l1, l2, mk, ncams, fw, fh, bw, bh, pitch, tiles_x, tiles_y, hdr, up, tune);
    CHECK(!up.desc.empty(), "no unit compiled");
    std::vector<int> cls_of(up.desc.size(), -1);
    for (int c = 0; c < kUnitClasses; ++c)
        for (uint32_t u : up.list[c]) cls_of[u] = c;
    // quads start at x % 4 == 0: unit left edges (unskewed) and the row skew are multiples of 4
    CHECK(up.skew == 0 || unit_skew(up.skew, 1) % 4 == 0, "skew constant %u", up.skew);
    for (size_t u = 0; u < up.desc.size(); ++u) {
        const int ux = (int)(int16_t)(up.desc[u].pos & 0xffffu);
        CHECK(((ux % 4) + 4) % 4 == 0, "unit %zu starts at column %d", u, ux);
        for (int y = 0; y < bh; ++y) CHECK(unit_skew(up.skew, y) % 4 == 0, "row %d skew %d", y, unit_skew(up.skew, y));
    }
    const int bw_own = std::min(pitch, tiles_x * 32);
    std::vector<uint8_t> claimed((size_t)pitch * bh, 0);
    size_t nclaimed = 0;
    for (int y = 0; y < bh; ++y)
        for (int x = 0; x < bw_own; ++x)
            claimed[(size_t)y * pitch + x] = (hdr[(size_t)(y / 8) * tiles_x + x / 32] & kHdrBlock) != 0;
    for (size_t t = 0; t < hdr.size(); ++t) nclaimed += (hdr[t] & kHdrBlock) != 0;

    const size_t img_bytes = (size_t)pitch * bh * 3 / 2;
    std::vector<uint8_t> img((size_t)nframes * img_bytes, 0), yw0, uvw0, bgr((size_t)pitch * bh * 3, 0);
    for (int b = 0; b < nframes; ++b) {
        std::vector<uint8_t> yw((size_t)pitch * bh, 0), uvw((size_t)(pitch / 2) * (bh / 2), 0);
        const UnitNv12Out nv = {img.data() + (size_t)b * img_bytes, bh, &yw, &uvw};
        for (size_t u = 0; u < up.desc.size(); ++u)
            unit_emulate(up, (uint32_t)u, cls_of[u], frames.data() + (size_t)b * set_bytes, set_bytes, blend != 0, has_car ? car_p.data() : nullptr,
                         pitch, bgr.data(), nullptr, nullptr, &nv);
        for (size_t i = 0; i < yw.size(); ++i) CHECK(yw[i] == claimed[i], "frame %d: Y byte (%zu, %zu) stored %d times (claimed %d)", b, i % pitch, i / pitch, yw[i], claimed[i]);
        for (int i = 0; i < bh / 2; ++i)
            for (int j = 0; j < pitch / 2; ++j)
                CHECK(uvw[(size_t)i * (pitch / 2) + j] == claimed[(size_t)(2 * i) * pitch + 2 * j], "frame %d: U / V pair of block (%d, %d) stored %d times", b, j, i,
                      uvw[(size_t)i * (pitch / 2) + j]);
        if (b == 0) { yw0 = yw; uvw0 = uvw; }
    }
    CHECK(std::all_of(bgr.begin(), bgr.end(), [](uint8_t v) { return v == 0; }), "the NV12 store stage wrote the BGR image");
    FILE *o = fopen(argv[2], "wb");
    CHECK(o, "cannot write %s", argv[2]);
    const int32_t oh[2] = {(int32_t)up.desc.size(), (int32_t)nclaimed};
    fwrite(oh, 4, 2, o);
    fwrite(claimed.data(), 1, claimed.size(), o);
    fwrite(yw0.data(), 1, yw0.size(), o);
    fwrite(uvw0.data(), 1, uvw0.size(), o);
    fwrite(img.data(), 1, img.size(), o);
    fclose(o);
    printf("nv12 store stage ok: %zu units, %zu of %zu base tiles, pitch %d\n", up.desc.size(), nclaimed, hdr.size(), pitch);
    return 0;
}
