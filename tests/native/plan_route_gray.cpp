// Host-only exhaustive check of the routing of a one-channel plan step (cameracalibration_amd/csrc/bevw_planapi.h: plan_route, frames_layout
// with SrcFormat::GRAY) -- runs without a GPU.  tests/native/plan_route_exhaustive.cpp holds the route of the four three-channel formats
// against the expressions it replaced; the channel count reaches the route as a fifth format and a sixth list, and this file states what
// they do, over every combination of the function's inputs (2^8 flags x 2^6 existing lists):
//   * one-channel frames are addressed by kLayoutGray, by the per-tap kernel and by the units;
//   * the units run exactly when the switch is on, the frames are 4-byte aligned, the one-channel list exists and the step is a plain one
//     (no balance, no channel sums, no compact scratch, no NV12 images); they then read whole frame sets (set_stride = set_bytes);
//   * no one-channel step writes NV12 images;
//   * whether the one-channel list exists changes nothing for the other four formats.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_planapi.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "plan route FAILED: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static RouteIn make(SrcFormat fmt, int bits, int have)
{
    RouteIn in;
    in.fmt = fmt;
    in.surf = bits & 1; in.out_nv12 = bits & 2; in.balance = bits & 4; in.sums = bits & 8; in.scratch = bits & 16;
    in.units_on = bits & 32; in.src_aligned = bits & 64; in.scratch_aligned = bits & 128;
    for (int l = 0; l < kPlanLayouts; ++l) in.have[l] = (have >> l) & 1;
    in.set_bytes = (uint32_t)(frame_bytes_of(320, 256, fmt) * 1); in.compact_stride = 123456u * 64u;
    return in;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    static_assert(kLayoutGray == kSrcLayouts && kPlanLayouts == kSrcLayouts + 1, "the one-channel layout stands behind the three-channel ones");
    CHECK(frame_bytes_of(320, 256, SrcFormat::GRAY) == 320u * 256u, "a one-channel frame is one byte per texel");
    CHECK(frames_layout(SrcFormat::GRAY, false) == kLayoutGray && frames_layout(SrcFormat::GRAY, true) == kLayoutGray, "frames_layout");
    unsigned long long cases = 0;
    for (int bits = 0; bits < 1 << 8; ++bits)
        for (int have = 0; have < 1 << kPlanLayouts; ++have) {
            const RouteIn in = make(SrcFormat::GRAY, bits, have);
            const Route r = plan_route(in);
            const bool plain = !in.balance && !in.sums && !in.scratch && !in.out_nv12;
            const bool use_units = in.units_on && in.src_aligned && in.have[kLayoutGray] && plain;
            CHECK(r.frames == kLayoutGray, "frames layout %d (bits %d have %d)", (int)r.frames, bits, have);
            CHECK(r.units == (in.scratch ? kLayoutCompact : kLayoutGray), "units layout %d (bits %d have %d)", (int)r.units, bits, have);
            CHECK(r.use_units == use_units, "use_units %d, expected %d (bits %d have %d)", r.use_units, use_units, bits, have);
            CHECK(!r.out_nv12, "NV12 images in one channel (bits %d have %d)", bits, have);
            CHECK(r.set_stride == (use_units ? in.set_bytes : 0u), "set_stride %u (bits %d have %d)", r.set_stride, bits, have);
            ++cases;
        }
    printf("gray route ok: %llu cases\n", cases);
    cases = 0;
    for (SrcFormat fmt : {SrcFormat::BGR, SrcFormat::NV12, SrcFormat::YUYV, SrcFormat::UYVY})
        for (int bits = 0; bits < 1 << 8; ++bits)
            for (int have = 0; have < 1 << kSrcLayouts; ++have) {
                const Route a = plan_route(make(fmt, bits, have)), b = plan_route(make(fmt, bits, have | (1 << kLayoutGray)));
                CHECK(a.frames == b.frames && a.units == b.units && a.use_units == b.use_units && a.out_nv12 == b.out_nv12 && a.set_stride == b.set_stride &&
                      a.lum == b.lum && a.tap_sums == b.tap_sums, "the one-channel list changes the route of format %d (bits %d have %d)", (int)fmt, bits, have);
                ++cases;
            }
    printf("other formats ok: %llu cases\n", cases);
    return 0;
}
