// Host-only check of the group loads of the unit kernel's SURFACE instantiation (cameracalibration_amd/csrc/bevw_unit.h:
// plan_unit_run<.., kLayoutSurf>, unit_gsrc_surf) -- runs without a GPU.  The plan compiler (unit_compile) builds the units of real tables; their
// group lists are translated for packed NV12 frame sets (unit_gsrc_nv12) and for surfaces with a row pitch (unit_gsrc_surf).  Random NV12
// frames are laid out twice: packed, and as surfaces inside an arena whose gaps and padding columns hold other bytes.  For every unit,
// round and lane the program walks the kernel's steps -- camera A / split / camera B of the wave's 64 lanes, one descriptor per plane
// (base, num_records = the plane's bytes), two 8-byte loads checked dword by dword as the buffer hardware checks them -- and verifies:
//   (a) every dword of every load lies wholly inside the plane of its descriptor or wholly outside the descriptor's range (zeros, no
//       memory touched): none straddles the end of a plane;
//   (b) the pair entries that land in the patch equal what the packed translation lands for the same frames (the bytes of texel x + 4 of
//       a row's last group excepted: that texel lies outside the frame and no unit pixel samples it);
//   (c) every group is fetched from the camera the BGR list names.
//
//   nv12_surf_emulate <in> <pitch>
//   in: int32 fw fh bw bh ncams 0 0 0 | per camera int16 lut1[bh][bw][2], uint16 lut2[bh][bw], uint8 mask[bh][bw]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

// one dword of a raw buffer load: descriptor (base inside `mem`, num_records), byte offset.  Returns 0 inside, 1 out of range as a whole, 2 straddling.
static int buffer_dword(const std::vector<uint8_t> &mem, size_t base, uint32_t num_records, uint32_t off, uint32_t &v)
{
    v = 0;
    if ((uint64_t)off + 4 <= num_records) { memcpy(&v, mem.data() + base + off, 4); return 0; }
    return off >= num_records ? 1 : 2;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    CHECK(argc == 3, "usage: nv12_surf_emulate <in> <pitch>");
    FILE *f = fopen(argv[1], "rb");
    CHECK(f, "cannot read %s", argv[1]);
    int32_t head[8];
    CHECK(fread(head, 4, 8, f) == 8, "short header");
    const int fw = head[0], fh = head[1], bw = head[2], bh = head[3], ncams = head[4];
    const int pitch = atoi(argv[2]);
    CHECK(fw % 4 == 0 && fh % 2 == 0 && pitch >= fw && pitch % 4 == 0 && ncams >= 1 && ncams <= 4, "geometry %d x %d, pitch %d", fw, fh, pitch);
    const size_t npx = (size_t)bw * bh;
    std::vector<int16_t> l1[4];
    std::vector<uint16_t> l2[4];
    std::vector<uint8_t> mk[4];
    for (int c = 0; c < ncams; ++c) {
        l1[c].resize(npx * 2); l2[c].resize(npx); mk[c].resize(npx);
        CHECK(fread(l1[c].data(), 2, npx * 2, f) == npx * 2 && fread(l2[c].data(), 2, npx, f) == npx && fread(mk[c].data(), 1, npx, f) == npx, "short tables");
    }
    fclose(f);

    const int tiles_x = (bw + 31) / 32, tiles_y = (bh + 7) / 8;
    std::vector<uint32_t> hdr = unit_host_headers(l1, mk, ncams, fw, fh, bw, bh, tiles_x, tiles_y);
    UnitPlanHost up;
    UnitTuning tune;
    tune.wide_double = 1;   // as plan_build
    unit_compile(l1, l2, mk, ncams, fw, fh, bw, bh, (bw + 3) & ~3, tiles_x, tiles_y, hdr, up, tune);
    CHECK(!up.desc.empty(), "no unit compiled");
    std::vector<int> cls_of(up.desc.size(), -1);
    for (int c = 0; c < kUnitClasses; ++c)
        for (uint32_t u : up.list[c]) cls_of[u] = c;
    std::vector<uint32_t> g_nv, g_sf;
    unit_gsrc_nv12(up.gsrc, fw, fh, g_nv);
    const std::vector<uint32_t> ranges = unit_slot_ranges(up);
    CHECK(unit_gsrc_surf(up.gsrc, fw, fh, pitch, g_sf, &ranges), "a unit names more than two cameras, or names them out of order");
    CHECK(g_nv.size() == up.gsrc.size() * 2 && g_sf.size() == up.gsrc.size() * 2, "list sizes");

    // the frames: packed NV12 frame set, and the same frames as surfaces in an arena (planes in scrambled order, U / V below Y for odd cameras,
    // gaps of varying size; gaps and padding columns hold the complement of a counter, never a frame's bytes by construction of the check below)
    const uint32_t y_bytes = (uint32_t)fw * fh, nv_frame = y_bytes / 2 * 3, y_plane = (uint32_t)pitch * fh, uv_plane = y_plane / 2;
    const size_t set_bytes = (size_t)nv_frame * ncams;
    std::vector<uint8_t> packed(set_bytes);
    uint32_t lcg = 12345u;
    for (uint8_t &b : packed) { lcg = lcg * 1664525u + 1013904223u; b = (uint8_t)(lcg >> 24); }
    size_t ybase[4], cbase[4], pos = 4096;
    const int order[4] = {2, 0, 3, 1};
    std::vector<int> cams;
    for (int k = 0; k < 4; ++k) if (order[k] < ncams) cams.push_back(order[k]);
    for (size_t k = 0; k < cams.size(); ++k) {
        const int c = cams[k];
        pos += 4 * (size_t)(37 + 101 * k);
        if (c & 1) { cbase[c] = pos; pos += uv_plane; pos += 4 * (size_t)(11 + 7 * k); ybase[c] = pos; pos += y_plane; }
        else { ybase[c] = pos; pos += y_plane; pos += 4 * (size_t)(5 + 13 * k); cbase[c] = pos; pos += uv_plane; }
    }
    std::vector<uint8_t> arena(pos + 4096);
    for (uint8_t &b : arena) { lcg = lcg * 1664525u + 1013904223u; b = (uint8_t)(lcg >> 24); }
    for (int c = 0; c < ncams; ++c) {
        for (int y = 0; y < fh; ++y) memcpy(arena.data() + ybase[c] + (size_t)y * pitch, packed.data() + (size_t)c * nv_frame + (size_t)y * fw, (size_t)fw);
        for (int y = 0; y < fh / 2; ++y)
            memcpy(arena.data() + cbase[c] + (size_t)y * pitch, packed.data() + (size_t)c * nv_frame + y_bytes + (size_t)y * fw, (size_t)fw);
    }

    const uint32_t frame_bytes = (uint32_t)fw * fh * 3, row_bytes = (uint32_t)fw * 3;
    size_t groups = 0, dw_in = 0, dw_out = 0, mixed = 0, two_cam_units = 0, rounds = 0;
    for (size_t u = 0; u < up.desc.size(); ++u) {
        const UnitDesc &d = up.desc[u];
        if (d.groups == 0) continue;
        const int GR = kUnitClassGR[cls_of[u]];
        uint32_t unit_cams = 0;
        for (int r = 0; r < GR; ++r)
            for (int wave = 0; wave < kUnitWaves; ++wave) {
                const size_t s0 = ((size_t)d.gs_off + r) * kUnitThreads + (size_t)wave * 64;
                // the descriptor pair each lane loads through, per round: camera A = the first lane's with a group, from lane `split` on camera B
                // (the kernel keeps A and B per wave and split per round: the same pair for every lane, as a unit names at most two cameras)
                uint32_t cam_a = 0, cam_b = 0, split = 64;
                bool any = false;
                for (int lane = 0; lane < 64; ++lane) {
                    if (g_sf[2 * (s0 + lane)] == kPairNoGroup) continue;
                    const uint32_t cam = unit_surf_cam(g_sf[2 * (s0 + lane) + 1]);
                    if (!any) { cam_a = cam; any = true; }
                    else if (cam != cam_a && split == 64) { split = (uint32_t)lane; cam_b = cam; }
                }
                if (split == 64) cam_b = cam_a;
                ++rounds;
                mixed += split < 64;
                for (int lane = 0; lane < 64; ++lane) {
                    const size_t i = s0 + lane;
                    const bool has = g_sf[2 * i] != kPairNoGroup;
                    CHECK(has == (up.gsrc[i] != kPairNoGroup) && has == (g_nv[2 * i] != kPairNoGroup), "unit %zu slot %zu: group / no group", u, i);
                    const uint32_t cam = (uint32_t)lane < split ? cam_a : cam_b;   // the descriptor pair this lane loads through
                    const uint32_t yo = g_sf[2 * i], co = has ? unit_surf_uv(g_sf[2 * i + 1]) : kPairNoGroup;
                    uint32_t w[4], p[4];
                    const int k0 = buffer_dword(arena, ybase[cam], y_plane, yo, w[0]), k1 = buffer_dword(arena, ybase[cam], y_plane, yo + 4, w[1]);
                    const int k2 = buffer_dword(arena, cbase[cam], uv_plane, co, w[2]), k3 = buffer_dword(arena, cbase[cam], uv_plane, co + 4, w[3]);
                    CHECK(k0 != 2 && k1 != 2 && k2 != 2 && k3 != 2, "unit %zu slot %zu: a dword straddles the end of a plane (offsets %u, %u)", u, i, yo, co);
                    if (!has) {
                        CHECK(k0 == 1 && k1 == 1 && k2 == 1 && k3 == 1, "unit %zu slot %zu: a lane without a group touches memory", u, i);
                        continue;
                    }
                    // (a) the first dword of each load holds sampled texels: inside its plane; the second is inside or out of range as a whole
                    CHECK(k0 == 0 && k2 == 0, "unit %zu slot %zu: the group's own dword is out of range (offsets %u, %u)", u, i, yo, co);
                    dw_in += 2 + (k1 == 0) + (k3 == 0);
                    dw_out += (k1 == 1) + (k3 == 1);
                    // (c) the camera the BGR list names
                    const uint32_t want_cam = up.gsrc[i] / frame_bytes, t = up.gsrc[i] % frame_bytes, y = t / row_bytes, x = t % row_bytes / 3;
                    CHECK(cam == want_cam && unit_surf_cam(g_sf[2 * i + 1]) == want_cam, "unit %zu slot %zu: fetched from camera %u, the plan names %u", u, i, cam, want_cam);
                    CHECK(yo == y * (uint32_t)pitch + x && co == (y >> 1) * (uint32_t)pitch + x, "unit %zu slot %zu: offsets", u, i);
                    unit_cams |= 1u << cam;
                    // (b) what lands: against the packed translation (its loads through the frame set's descriptor)
                    const std::vector<uint8_t> &pk = packed;
                    buffer_dword(pk, 0, (uint32_t)set_bytes, g_nv[2 * i], p[0]); buffer_dword(pk, 0, (uint32_t)set_bytes, g_nv[2 * i] + 4, p[1]);
                    buffer_dword(pk, 0, (uint32_t)set_bytes, g_nv[2 * i + 1], p[2]); buffer_dword(pk, 0, (uint32_t)set_bytes, g_nv[2 * i + 1] + 4, p[3]);
                    uint4 A, B, PA, PB;
                    pair_convert_nv12(w[0], w[1], w[2], w[3], true, A, B);
                    pair_convert_nv12(p[0], p[1], p[2], p[3], true, PA, PB);
                    uint8_t e[32], pe[32];
                    memcpy(e, &A, 16); memcpy(e + 16, &B, 16); memcpy(pe, &PA, 16); memcpy(pe + 16, &PB, 16);
                    const bool row_end = x + 4 == (uint32_t)fw;   // pair 3 = texels x + 3, x + 4: bytes 1, 3, 5 of it are texel x + 4, outside the frame
                    for (int b = 0; b < 32; ++b) {
                        if (row_end && b >= 24 && (b == 25 || b == 27 || b == 29)) continue;
                        CHECK(e[b] == pe[b], "unit %zu slot %zu (camera %u, texel %u, %u): patch byte %d is %u, the packed kernel lands %u", u, i, cam, x, y, b, e[b], pe[b]);
                    }
                    ++groups;
                }
            }
        two_cam_units += (unit_cams & (unit_cams - 1)) != 0;
    }
    printf("surface loads ok: units %zu two_camera_units %zu groups %zu wave_rounds %zu mixed_rounds %zu dwords_inside %zu dwords_out_of_range %zu pitch %d\n",
           up.desc.size(), two_cam_units, groups, rounds, mixed, dw_in, dw_out, pitch);
    return 0;
}
