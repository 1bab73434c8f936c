// Host-only check of the packed 4:2:2 landing of the unit kernel (cameracalibration_amd/csrc: bevw_unit.h unit_gsrc_yuv422, bevw_pair.h
// pair_convert_yuv422, bevw_device.h yuv422_order) -- runs without a GPU.  The kernels' own __host__ __device__ functions are compiled for
// the host and their results written to files; tests/test_yuv422_host.py compares them with the NumPy specification (tests/_yuv422_spec.py).
//
//   yuv422_emulate land ORDER FW FH NCAMS SET GSRC OFFS PAIRS
//       ORDER: 4 = YUYV, 5 = UYVY (BEVW_INPUT_*).  SET: a packed 4:2:2 frame set (NCAMS frames of FW x FH x 2 bytes); GSRC: uint32 group
//       list as the unit plan holds it (BGR frame-set offsets 12 k, kPairNoGroup for lanes without a group).  Writes OFFS =
//       unit_gsrc_yuv422(GSRC) and PAIRS = per slot the 32 bytes the unit kernel's 4:2:2 instantiation lands in its LDS patch: ONE 16-byte
//       load at the slot's offset (dwords past the frame set read as 0, as the buffer's range check returns them; the program fails on a
//       dword that straddles the end of the set; a lane without a group loads nothing) -> pair_convert_yuv422 with the order's selectors.
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

static int land(int order, int fw, int fh, int ncams, const char *set_path, const char *gsrc_path, const char *offs_path, const char *pairs_path)
{
    if (order != (int)SrcFormat::YUYV && order != (int)SrcFormat::UYVY) { printf("bad order\n"); return 2; }
    std::vector<uint8_t> set, graw;
    if (!read_file(set_path, set) || !read_file(gsrc_path, graw)) return 2;
    if (set.size() != frame_bytes_of(fw, fh, (SrcFormat)order) * (size_t)ncams || graw.size() % 4) { printf("bad input sizes\n"); return 2; }
    std::vector<uint32_t> gsrc(graw.size() / 4), offs;
    memcpy(gsrc.data(), graw.data(), graw.size());
    unit_gsrc_yuv422(gsrc, fw, fh, offs);
    const Yuv422Order sel = yuv422_order((SrcFormat)order);
    std::vector<uint32_t> pairs(gsrc.size() * 8);
    for (size_t i = 0; i < gsrc.size(); ++i) {
        uint32_t w[4] = {0, 0, 0, 0};
        const bool has = offs[i] != kPairNoGroup;
        if (has) {   // raw buffer load of 4 dwords, num_records = the frame set's bytes: a dword is inside as a whole or returns 0
            if (offs[i] % 4) { printf("slot %zu: offset %u is not dword-aligned\n", i, offs[i]); return 1; }
            for (int d = 0; d < 4; ++d) {
                const size_t o = (size_t)offs[i] + 4 * d;
                if (o + 4 <= set.size()) memcpy(&w[d], &set[o], 4);
                else if (o < set.size()) { printf("slot %zu: dword %d straddles the end of the frame set\n", i, d); return 1; }
            }
        }
        uint4 A, B;
        pair_convert_yuv422(w[0], w[1], w[2], w[3], sel, has, A, B);
        const uint32_t e[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        memcpy(&pairs[i * 8], e, 32);
    }
    if (!write_file(offs_path, offs.data(), offs.size() * 4) || !write_file(pairs_path, pairs.data(), pairs.size() * 4)) return 2;
    printf("yuv422 land ok: %zu slots\n", gsrc.size());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    if (argc == 10 && strcmp(argv[1], "land") == 0)
        return land(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6], argv[7], argv[8], argv[9]);
    fprintf(stderr, "usage: yuv422_emulate land ORDER FW FH NCAMS SET GSRC OFFS PAIRS\n");
    return 2;
}
