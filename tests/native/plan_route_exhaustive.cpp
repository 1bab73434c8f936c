// Host-only exhaustive check of the routing of a plan step (cameracalibration_amd/csrc/bevw_planapi.h: plan_route, frames_layout) -- runs
// without a GPU.
//
// plan_route decides which group list the units of a step read, whether the units may run, whether the step writes NV12 images, the set
// stride and the LUM / SUMS flags of the per-tap kernel.  It replaced expressions that were spread over plan_stitch_impl and plan_lum_band;
// those expressions are written out below as the SPECIFICATION (named as they were: out_nv12, compact, nv12_units, yuv422_units, use_units,
// the list chosen, set_stride, LUM / SUMS), and every combination of the function's inputs is held against them:
//   4 formats x surfaces x NV12 images x balance x sums x scratch x units switch x 2 alignments x 2^5 existing lists = 32768 cases.
// The sampled-group list of plan_lum_band is held against its former ladder for the 8 (format, surfaces) pairs; the pair (4:2:2, surfaces),
// which no entry point lets through (surfaces are NV12), is the one place where the two former functions disagreed with each other -- the
// ladder took the surface list, the launch below it the 4:2:2 kernel -- and frames_layout follows the kernel.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_planapi.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "plan route FAILED: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static const SrcFormat kFormats[4] = {SrcFormat::BGR, SrcFormat::NV12, SrcFormat::YUYV, SrcFormat::UYVY};
// frame sets of 320 x 256 texels, four cameras: the strides only have to differ from each other
constexpr int kFW = 320, kFH = 256, kCams = 4;
constexpr uint32_t kCompactStride = 123456u * 64u;

static int check_route(const RouteIn &in)
{
    const Route r = plan_route(in);
    // ---- the specification: the expressions of plan_stitch_impl before plan_route ----
    const bool nv12 = in.fmt == SrcFormat::NV12, yuv422 = src_is_yuv422(in.fmt), surf = in.surf;
    const bool out_nv12 = in.out_nv12 && !in.balance && !in.sums && !in.scratch;
    const bool compact = in.scratch;
    const bool nv12_units = nv12 && !compact;
    const bool yuv422_units = yuv422 && !compact;
    const bool use_units = !in.balance && in.units_on && in.src_aligned &&
                           (!compact || (in.have[kLayoutCompact] && in.scratch_aligned)) &&
                           (!nv12_units || ((surf ? in.have[kLayoutSurf] : in.have[kLayoutNV12]) && !in.sums)) &&
                           (!yuv422_units || (in.have[kLayoutYuv422] && !in.sums));
    // the list the units read (a.un_gsrc), the last assignment winning as it did
    SrcLayout list = kLayoutBGR;
    uint32_t set_stride = 0;
    if (compact) { list = kLayoutCompact; set_stride = in.compact_stride; }
    if (nv12_units) { list = surf ? kLayoutSurf : kLayoutNV12; set_stride = (uint32_t)(frame_bytes_of(kFW, kFH, true) * kCams); }
    if (yuv422_units) { list = kLayoutYuv422; set_stride = (uint32_t)(frame_bytes_of(kFW, kFH, in.fmt) * kCams); }
    // the unit kernel's <NV12, SURF, P422> as plan_launch_units was handed them
    const bool k_nv12 = nv12_units, k_surf = surf && nv12_units, k_yuv422 = yuv422_units;
    // the per-tap kernel: k_stitch_plan_yuv422, or with_layout_out(rt.frames, ..) on the three other frame layouts
    const SrcLayout tap = yuv422 ? kLayoutYuv422 : surf ? kLayoutSurf : nv12 ? kLayoutNV12 : kLayoutBGR;
    const bool lum = in.balance || compact, tap_sums = in.balance || in.sums;
    // ---- plan_route against it ----
#define WHERE "fmt %d surf %d out_nv12 %d balance %d sums %d scratch %d units_on %d aligned %d/%d have %d%d%d%d%d"
#define ARGS (int)in.fmt, in.surf, in.out_nv12, in.balance, in.sums, in.scratch, in.units_on, in.src_aligned, in.scratch_aligned, in.have[0], in.have[1], in.have[2], in.have[3], in.have[4]
    CHECK(r.out_nv12 == out_nv12, "out_nv12 %d, was %d: " WHERE, r.out_nv12, out_nv12, ARGS);
    CHECK(r.use_units == use_units, "use_units %d, was %d: " WHERE, r.use_units, use_units, ARGS);
    CHECK((r.units == kLayoutCompact) == compact, "compact %d, was %d: " WHERE, r.units == kLayoutCompact, compact, ARGS);
    CHECK((r.units == kLayoutNV12 || r.units == kLayoutSurf) == k_nv12 && (r.units == kLayoutSurf) == k_surf && (r.units == kLayoutYuv422) == k_yuv422,
          "unit kernel of layout %d, was nv12 %d surf %d yuv422 %d: " WHERE, (int)r.units, k_nv12, k_surf, k_yuv422, ARGS);
    CHECK(r.units == list, "list %d, was %d: " WHERE, (int)r.units, (int)list, ARGS);
    if (use_units) CHECK(r.set_stride == set_stride, "set_stride %u, was %u: " WHERE, r.set_stride, set_stride, ARGS);
    else CHECK(r.set_stride == 0, "set_stride %u without units: " WHERE, r.set_stride, ARGS);
    CHECK(r.frames == tap, "per-tap kernel of layout %d, was %d: " WHERE, (int)r.frames, (int)tap, ARGS);
    CHECK(r.lum == lum && r.tap_sums == tap_sums, "LUM %d SUMS %d, were %d %d: " WHERE, r.lum, r.tap_sums, lum, tap_sums, ARGS);
    // what the dispatch relies on: NV12 images carry neither flag, and a list the units read exists
    CHECK(!r.out_nv12 || (!r.lum && !r.tap_sums), "NV12 images with LUM / SUMS: " WHERE, ARGS);
    CHECK(!r.use_units || r.units == kLayoutBGR || in.have[r.units], "units on a list that does not exist: " WHERE, ARGS);
#undef WHERE
#undef ARGS
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    unsigned long long cases = 0;
    for (SrcFormat fmt : kFormats)
        for (int bits = 0; bits < 1 << 8; ++bits)
            for (int have = 0; have < 1 << kSrcLayouts; ++have) {
                RouteIn in;
                in.fmt = fmt;
                in.surf = bits & 1; in.out_nv12 = bits & 2; in.balance = bits & 4; in.sums = bits & 8; in.scratch = bits & 16;
                in.units_on = bits & 32; in.src_aligned = bits & 64; in.scratch_aligned = bits & 128;
                for (int l = 0; l < kSrcLayouts; ++l) in.have[l] = (have >> l) & 1;
                in.set_bytes = (uint32_t)(frame_bytes_of(kFW, kFH, fmt) * kCams); in.compact_stride = kCompactStride;
                if (check_route(in)) return 1;
                ++cases;
            }
    printf("plan route ok: %llu cases\n", cases);
    // the sampled-group list of plan_lum_band: surfaces, else NV12, else 4:2:2, else BGR
    cases = 0;
    for (SrcFormat fmt : kFormats)
        for (int surf = 0; surf < 2; ++surf) {
            const SrcLayout was = surf ? kLayoutSurf : fmt == SrcFormat::NV12 ? kLayoutNV12 : src_is_yuv422(fmt) ? kLayoutYuv422 : kLayoutBGR;
            const SrcLayout now = frames_layout(fmt, surf != 0);
            if (surf && src_is_yuv422(fmt)) CHECK(now == kLayoutYuv422, "4:2:2 frames follow their kernel, got layout %d", (int)now);
            else CHECK(now == was, "sampled list %d, was %d: fmt %d surf %d", (int)now, (int)was, (int)fmt, surf);
            ++cases;
        }
    printf("sampled list ok: %llu cases\n", cases);
    return 0;
}
