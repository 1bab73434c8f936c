// bevw_planapi.h -- what the rest of the library sees of the tile plan: the Plan a handle owns, the tables it is compiled from and the
// entry points with their arguments (FrameSource, PlanStep).  No kernels: the plan kernels (bevw_plan.h, bevw_unit.h) are compiled in
// bevwarp_plan.hip alone, which defines every function declared here.  Every plan_* function that returns an int returns a BEVW_* status and leaves its message in bevw_last_error().
#pragma once
#include "bevw_device.h"   // Nv12Surface, HsvTables, SrcFormat, SrcLayout, frame_bytes_of
#include "bevw_host.h"

namespace bevw {

// Static tables of one BevGenerator as the per-pixel schedule and the plan compiler read them.
struct StitchTables {
    const int16_t *lut1[4];
    const uint16_t *lut2[4];
    const uint8_t *mask[4];
};

// Where the camera frames of a step are.  Packed: `packed` points at frame sets of `cams` dense frames of format `fmt`.  Surfaces: `surf` is a
// device table surf[frame set][cams] of NV12 surfaces with rows of `pitch` bytes, which every kernel reads in place; `packed` is then nullptr
// and is never read.
struct FrameSource {
    const uint8_t *packed = nullptr;
    const Nv12Surface *surf = nullptr;
    int pitch = 0;       // bytes between the rows of a surface
    SrcFormat fmt = SrcFormat::BGR;
    int cams = 4;        // frames per set: 4 for a BevGenerator, 1 for a remapper or a list of single frames
    bool is_surf() const { return surf != nullptr; }
    bool nv12() const { return fmt == SrcFormat::NV12; }
    bool yuv422() const { return src_is_yuv422(fmt); }   // packed 4:2:2 (YUYV / UYVY): never surfaces
    size_t set_bytes(int fw, int fh) const { return frame_bytes_of(fw, fh, fmt) * (size_t)cams; }
    bool aligned4() const { return (((uintptr_t)packed) & 3u) == 0; }   // dword loads (a surface's planes were checked when its table was staged)
    FrameSource from(int b0, int fw, int fh) const   // the source of frame set b0 onward
    {
        FrameSource s = *this;
        if (surf) s.surf += (size_t)b0 * cams;
        else s.packed += (size_t)b0 * set_bytes(fw, fh);
        return s;
    }
};

// What a group list addresses (SrcLayout, bevw_device.h).  Every list of the plan -- the units' group lists and the sampled groups of the
// balance schedule -- exists once per layout of the memory it is read against: packed BGR, packed NV12, NV12 surfaces at Plan::src_pitch,
// packed 4:2:2, the compact scratch (DESIGN.md section 8 has the table: what a slot holds, when a list is made, when it is missing).  A
// missing list is nullptr, which sends the step to the per-tap kernel and is never an error.
// kLayoutGray: the one-channel frames of a remapper or a handle (SrcFormat::GRAY), 1 byte per texel: the units' list alone, no sampled list
// (no balance schedule), and routed by the format alone.  SrcFormat::GRAY16 (bevw_remapper_set_depth) reads the same list: a group's offset
// in 2 bytes per texel is twice its offset in 1.

// a compiled tile plan: its device buffers and the geometry they were built for (plan_build / plan_build_wide)
struct Plan {
    void *entries = nullptr;     // uint2[ntiles][8][64]
    void *hdr = nullptr;         // uint32[ntiles]
    void *psums = nullptr;       // uint32[batch][ntiles][3]  (balance: per-tile channel sums)
    size_t psums_cap = 0;
    int psums_layout = -1;       // entries per frame of the layout the last plan_stitch call with sums wrote (plan_sum_entries)
    // destination widths that are not a multiple of 4 pixels: the kernels' 12-byte stores need dword-aligned pixel quads,
    // so they write rows of `pitch` = bw rounded up to 4 pixels into pad_out and k_plan_unpad compacts them (one more
    // pass over the output instead of the per-pixel schedule)
    int pitch = 0;
    bool out_pitched = false;    // the caller's output images have rows of `pitch` pixels themselves (bevw_set_output_pitch): no scratch, no compaction
    void *pad_out = nullptr, *pad_car = nullptr;
    void *pad_car_gray = nullptr;   // one channel: the car sprite at the images' pitch (a pitched handle with bw % 4 != 0: plan_gray_stitch_step)
    size_t pad_cap = 0;
    int *d_max = nullptr;
    int fw = 0, fh = 0, bw = 0, bh = 0;
    int tiles_x = 0, tiles_y = 0, ntiles = 0;
    int ncams = 4;
    // the group lists, one per layout of what they address (SrcLayout; bevw_unit.h has the translations).  sampled: the n_groups sampled
    // 4-texel groups of the frame set in ascending order (balance schedule 1: plan_lum_groups; none for the compact scratch it writes)
    void *units[kPlanLayouts] = {}, *sampled[kPlanLayouts] = {};
    int n_groups = 0;
    bool band_ok = false;        // the sampled-group list exists (balance schedule 1)
    int max_contrib = 0;
    bool usable = false;
    void *list_slow = nullptr;   // base tiles no unit owns (frame-border footprints; everything when there are no units)
    int n_slow = 0;
    // unit schedule (bevw_unit.h): k-d partition compiled on the host
    void *un_desc = nullptr, *un_entries = nullptr;
    size_t compact_stride = 0;               // bytes between the compact scratch copies of consecutive frame sets (0: units[kLayoutCompact] does not exist)
    void *list_un_all = nullptr;             // every unit in partition order, class in bits 28..31
    int n_un_all = 0;
    int n_un[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // units per class (diagnostics)
    int n_unit_tiles = 0;                    // base tiles the units own
    size_t un_lines = 0, un_sectors = 0;     // request arithmetic of the partition (per frame)
    int un_skew = 0;
    // The formats of the plan's steps, written by plan_set_format alone (plan_build resets them).  fmt: what their frame sets hold (bevw_set_input_format).
    SrcFormat fmt = SrcFormat::BGR;
    // out_nv12: they write NV12 images of `pitch` bytes per row (bevw_set_output_format; needs pitch % 4 == 0 and no padded scratch).  Steps
    // with channel sums (balance) still write the BGR pre-gain image: their gain pass converts.
    bool out_nv12 = false;
    // src_pitch: NV12 surfaces (bevw_set_input_pitch / bevw_run_surfaces_device) have rows of src_pitch bytes: the pitch the kLayoutSurf lists
    // are translated for (0: none).  The host copies of the BGR lists every translation starts from stay with the plan.
    int src_pitch = 0;
    std::vector<uint32_t> un_gsrc_host, groups_host, un_ranges_host;   // (un_ranges_host: first slot and slot count of every unit's list)
};

// The routing of one step of the plan: which list the units read, whether they may run, and what is left to the per-tap kernel.  Pure host
// arithmetic and the one place that knows these rules (plan_stitch and plan_lum_groups ask it; tests/native/plan_route_exhaustive.cpp holds
// it against the expressions it replaced, for every input).
struct RouteIn {
    SrcFormat fmt = SrcFormat::BGR;   // the plan's format (Plan::fmt)
    bool surf = false;                // the step's frames are NV12 surfaces
    bool out_nv12 = false;            // the plan writes NV12 images (Plan::out_nv12)
    bool balance = false, sums = false, scratch = false;   // the step's (PlanStep; scratch: it brings a compact scratch)
    bool units_on = false;            // the units switch is on and the plan has units
    bool src_aligned = false, scratch_aligned = false;     // the frame sets / the compact scratch are 4-byte aligned
    bool have[kPlanLayouts] = {};     // Plan::units[layout] exists
    uint32_t set_bytes = 0, compact_stride = 0;   // bytes of one frame set in the plan's format; Plan::compact_stride
};
struct Route {
    SrcLayout frames;      // how the step's frames are addressed: the per-tap kernel's instantiation, the sampled list of k_lum_groups
    SrcLayout units;       // what the units read: the frames, or the BGR compact scratch
    bool use_units;        // the units run, the per-tap kernel serves only what no unit owns; false: it serves every tile
    bool out_nv12;         // the step writes NV12 images: never one that leaves a pre-gain BGR image (channel sums) or serves a shard (scratch)
    uint32_t set_stride;   // PlanArgs::set_stride of the units (0: dense BGR frame sets)
    bool lum, tap_sums;    // the LUM / SUMS flags of the per-tap kernel
};
inline SrcLayout frames_layout(SrcFormat fmt, bool surf)
{
    return src_is_gray(fmt) ? kLayoutGray : src_is_yuv422(fmt) ? kLayoutYuv422 : surf ? kLayoutSurf : fmt == SrcFormat::NV12 ? kLayoutNV12 : kLayoutBGR;
}
inline Route plan_route(const RouteIn &in)
{
    Route r;
    r.frames = frames_layout(in.fmt, in.surf);
    // the units read the compact scratch where the step brings one, else the frames (surfaces are NV12: any other format with a surface
    // table is refused before a step gets here, and routed as its packed frames)
    r.units = in.scratch ? kLayoutCompact : frames_layout(in.fmt, in.surf && in.fmt == SrcFormat::NV12);
    const bool bgr_units = r.units == kLayoutBGR || r.units == kLayoutCompact;
    // the units need their list, 4-byte aligned memory behind it (dword-addressed group loads), and are not combined with the per-tap
    // luminance kernel (balance); channel sums exist with BGR units only.  (The BGR list exists wherever the plan has units.)
    r.use_units = !in.balance && in.units_on && in.src_aligned && (r.units == kLayoutBGR || in.have[r.units]) &&
                  (r.units != kLayoutCompact || in.scratch_aligned) && (bgr_units || !in.sums);
    // one channel: the units on the frames themselves or nothing -- no balance chain, no shard scratch, no NV12 image exists in one channel,
    // and a step without units leaves the plan (the caller runs the per-pixel kernel: plan_units_serve)
    const bool gray = src_is_gray(in.fmt);   // (16 bits: the same list and the same rules -- k_units_gray16 doubles the list's offsets)
    if (gray) r.use_units = r.use_units && r.units == kLayoutGray && !in.out_nv12;
    r.out_nv12 = in.out_nv12 && !in.balance && !in.sums && !in.scratch && !gray;
    r.set_stride = !r.use_units || r.units == kLayoutBGR ? 0u : r.units == kLayoutCompact ? in.compact_stride : in.set_bytes;
    // LUM: luminance round trip per tap (the RAW frames of balance, or the tiles no unit owns beside the compact scratch); a scratch without
    // sums: camera-per-GPU shards, whose stitch rank balances the colours.  Neither exists with NV12 images (out_nv12 above)
    r.lum = in.balance || in.scratch;
    r.tap_sums = in.balance || in.sums;
    return r;
}

// compile LUT + masks into a plan (table kernels, unit compiler on the host).  out_pitch: pixels per output row when the caller's images
// are pitched (0: dense); blend: the handle applies blend weights (its units carry no two-quad two-contributor class)
int plan_build(Plan &p, hipStream_t st, const StitchTables &T, int fw, int fh, int bw, int bh, int ncams, int out_pitch, bool blend);

// One step of the tile plan (plan_stitch).  A field left at its default is not used.
struct PlanStep {
    FrameSource src;
    int batch = 0; bool blend = false;
    // luminance round trip per tap on RAW frames (the per-tap kernel over every tile) + per-tile channel sums
    bool balance = false;
    // per-unit / per-tile channel sums, the car left to the gain pass (with `scratch`; or: the frames are luminance-shifted already)
    bool sums = false;
    const int *deltas = nullptr; const HsvTables *tab = nullptr;   // balance / scratch: luminance deltas[frame set][4], the HSV divisor tables
    const uint8_t *car = nullptr; uint8_t *out = nullptr;
    // balance and sums end with k_reduce_psums into chsums[frame set][3]; nullptr: the caller's gain pass adds the partial sums itself (plan_sum_entries)
    unsigned long long *chsums = nullptr;
    // the psums buffer is sized for psums_frames frame sets and this step's start at slot psums_first of it (two half-batches of one balance
    // step run concurrently on two streams: balance_plan_run); 0: this step's batch alone
    int psums_frames = 0, psums_first = 0;
    // the compact scratch plan_lum_groups filled from the frames (balance schedule 1): the units read IT (p.compact_stride bytes per frame
    // set, group lists p.units[kLayoutCompact]), the per-tap kernel serves what no unit owns from the RAW frames with the luminance round trip per
    // tap (deltas, tab); everything on the per-tap kernel when the units cannot run
    const uint8_t *scratch = nullptr;
    // a one-channel remapper's step in nearest-neighbour mode (bevw_remapper_set_interpolation): the same route and lists on the kernels of
    // bevwarp_nearest.hip, at the plan's depth
    bool nearest = false;
};
int plan_stitch(Plan &p, hipStream_t st, const PlanStep &step);
// whether the unit kernel serves that step (plan_route on the plan's lists and the step's pointers): what a remapper records as the path of
// the step, and for one-channel frames whether the step may enter the plan at all
bool plan_units_serve(const Plan &p, const PlanStep &step);

// balance: luminance round trip of the sampled texel groups of the raw frames into the compact scratch (p.compact_stride bytes per frame set)
int plan_lum_groups(const Plan &p, hipStream_t st, const FrameSource &src, uint8_t *d_scratch, int batch, const int *d_deltas, const HsvTables *d_tab);

// The pixel formats of the plan's steps, and for NV12 surfaces the row pitch the group lists are translated for (0: none).  After plan_build,
// with no step queued.
int plan_set_format(Plan &p, SrcFormat fmt, bool out_nv12, int src_pitch);

// rows of bw pixels -> rows of pitch pixels (the car sprite of a pitched handle)
int plan_pad_image(hipStream_t st, const uint8_t *d_src, int bw, int pitch, int bh, uint8_t *d_dst);

// analytic projection modes: the WIDE unit plan compiled from the projection map of every camera (sxy: int16 [bh][bw][2] top-left texels,
// frac: uint32 [bh][bw][2] 21-bit fractions, mask: uint8 [bh][bw]; host copies), and its launch
int plan_build_wide(Plan &p, const std::vector<int16_t> sxy[4], const std::vector<uint32_t> frac[4], const std::vector<uint8_t> mask[4], int fw, int fh,
                    int bw, int bh, bool blend);
int plan_stitch_wide(const Plan &p, hipStream_t st, const uint8_t *d_frames, int batch, bool blend, const uint8_t *d_car, uint8_t *d_out);

// frees the plan's device buffers and leaves an empty Plan
void plan_release(Plan &p);

// the partial channel sums the last plan_stitch call with sums left for frame `first` of the psums buffer, and their number per frame
const uint32_t *plan_sum_entries(const Plan &p, int first, int &nsum);

}  // namespace bevw
