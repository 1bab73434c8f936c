// Host-only checks of the NV12 input path (cameracalibration_amd/csrc: bevw_device.h nv12_row_bgr, bevw_pair.h pair_convert_nv12,
// bevw_unit.h unit_gsrc_nv12) -- runs without a GPU.  The kernels' own __host__ __device__ functions are compiled for the host and their
// results written to files; tests/test_nv12_host.py compares them with the NumPy specification (tests/_nv12_spec.py).
//
//   nv12_exhaustive table OUT
//       BGR of every (Y, U, V), 2^24 x 3 bytes in (Y << 16 | U << 8 | V) order, through nv12_row_bgr<2> (the group conversion: two texels
//       sharing one U / V pair; the program fails when the two differ) and nv12_row_bgr<5>'s last texel.
//   nv12_exhaustive land FW FH NCAMS SET GSRC OFFS PAIRS
//       SET: an NV12 frame set (NCAMS frames of FW x FH); GSRC: uint32 group list as the unit plan holds it (BGR frame-set offsets 12 k,
//       kPairNoGroup for lanes without a group).  Writes OFFS = unit_gsrc_nv12(GSRC) and PAIRS = per slot the 32 bytes the unit kernel's
//       NV12 instantiation lands in its LDS patch: two 8-byte loads at the two offsets (bytes past the frame set read as 0, as the buffer's
//       range check returns them; a lane without a group loads nothing) -> pair_convert_nv12.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"

using namespace bevw;

static bool read_file(const char *path, std::vector<uint8_t> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    v.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    const bool ok = fread(v.data(), 1, v.size(), f) == v.size();
    fclose(f);
    return ok;
}
static bool write_file(const char *path, const void *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    fclose(f);
    return ok;
}

static int table(const char *out)
{
    std::vector<uint8_t> t((size_t)3 << 24);
    for (uint32_t y = 0; y < 256; ++y)
        for (uint32_t u = 0; u < 256; ++u)
            for (uint32_t v = 0; v < 256; ++v) {
                uint32_t P[2], Q[5];
                nv12_row_bgr<2>(y | (y << 8), u | (v << 8), P);
                // five texels: the last one takes U / V bytes 4, 5
                nv12_row_bgr<5>((uint64_t)y << 32, (uint64_t)(u | (v << 8)) << 32, Q);
                if (P[0] != P[1] || P[0] != Q[4] || (P[0] >> 24) != 0) {
                    printf("group conversion disagrees at Y %u U %u V %u: %06x %06x %06x\n", y, u, v, P[0], P[1], Q[4]);
                    return 1;
                }
                uint8_t *d = &t[(((size_t)y << 16) | (u << 8) | v) * 3];
                d[0] = (uint8_t)P[0]; d[1] = (uint8_t)(P[0] >> 8); d[2] = (uint8_t)(P[0] >> 16);
            }
    if (!write_file(out, t.data(), t.size())) return 2;
    printf("nv12 table ok: %zu triples\n", t.size() / 3);
    return 0;
}

static int land(int fw, int fh, int ncams, const char *set_path, const char *gsrc_path, const char *offs_path, const char *pairs_path)
{
    std::vector<uint8_t> set, graw;
    if (!read_file(set_path, set) || !read_file(gsrc_path, graw)) return 2;
    if (set.size() != (size_t)fw * fh * 3 / 2 * ncams || graw.size() % 4) { printf("bad input sizes\n"); return 2; }
    std::vector<uint32_t> gsrc(graw.size() / 4), offs;
    memcpy(gsrc.data(), graw.data(), graw.size());
    unit_gsrc_nv12(gsrc, fw, fh, offs);
    auto load8 = [&](uint32_t off, uint32_t w[2]) {   // raw buffer load of 8 bytes, num_records = the frame set's bytes
        uint8_t b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 8; ++k)
            if ((size_t)off + k < set.size()) b[k] = set[(size_t)off + k];
        memcpy(w, b, 8);
    };
    std::vector<uint32_t> pairs(gsrc.size() * 8);
    for (size_t i = 0; i < gsrc.size(); ++i) {
        uint32_t yw[2], cw[2];
        load8(offs[2 * i], yw);
        load8(offs[2 * i + 1], cw);
        uint4 A, B;
        pair_convert_nv12(yw[0], yw[1], cw[0], cw[1], offs[2 * i] != kPairNoGroup, A, B);
        const uint32_t e[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        memcpy(&pairs[i * 8], e, 32);
    }
    if (!write_file(offs_path, offs.data(), offs.size() * 4) || !write_file(pairs_path, pairs.data(), pairs.size() * 4)) return 2;
    printf("nv12 land ok: %zu slots\n", gsrc.size());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    if (argc == 3 && strcmp(argv[1], "table") == 0) return table(argv[2]);
    if (argc == 9 && strcmp(argv[1], "land") == 0) return land(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argv[5], argv[6], argv[7], argv[8]);
    fprintf(stderr, "usage: nv12_exhaustive table OUT | land FW FH NCAMS SET GSRC OFFS PAIRS\n");
    return 2;
}
