// Host-only census for tests/test_batch_loops_host.py -- runs without a GPU.
//
//   --moving-nb               moving_nb (cameracalibration_amd/csrc/bevw_moving.h) over batches 1 .. 520 x tile counts {1, 252, 4096, 73170}:
//                             nb is 1, 2, 4, 8 or 16, the blocks z = 0 .. ceil(batch / nb) - 1 own [z * nb, min(batch, z * nb + nb)) as
//                             k_stitch_moving cuts them, every range is non-empty and every frame set lies in exactly one of them
//   --moving-table TILES B .. prints "B nb blocks last_block_frame_sets" per batch B, one line each (the table the GPU batches of
//                             k_stitch_moving were chosen by)
//   --units <in>              unit_compile on a caller's map as the library compiles a one-camera plan (tests/native/gray_emulate.cpp):
//                             prints "units N empty E tiles T per_tap P" -- units, units without any contributor (UnitDesc::groups == 0:
//                             the `ngroups == 0` loop of the one-channel unit kernels), base tiles, base tiles no unit claimed (the per-tap
//                             kernels')
//                             in: int32 fw fh bw bh | int16 map1[bh][bw][2] | uint16 map2[bh][bw]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../cameracalibration_amd/csrc/bevw_plan.h"
#include "../../cameracalibration_amd/csrc/bevw_moving.h"

using namespace bevw;

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "batch loops census FAILED: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static int moving_enumerate()
{
    const long long tile_counts[4] = {1, 252, 4096, 73170};
    unsigned long long cases = 0;
    std::vector<int> owners;
    for (long long tiles : tile_counts)
        for (int batch = 1; batch <= 520; ++batch) {
            const int nb = moving_nb(batch, tiles);
            CHECK(nb == 1 || nb == 2 || nb == 4 || nb == 8 || nb == 16, "batch %d tiles %lld: nb %d", batch, tiles, nb);
            const int blocks = (batch + nb - 1) / nb;   // grid.z of moving_launch_stitch
            owners.assign(batch, 0);
            for (int z = 0; z < blocks; ++z) {
                const int b_begin = z * nb, b_end = batch < b_begin + nb ? batch : b_begin + nb;   // as the kernel cuts them
                CHECK(b_end > b_begin, "batch %d tiles %lld nb %d: block %d is empty", batch, tiles, nb, z);
                for (int b = b_begin; b < b_end; ++b) ++owners[b];
            }
            for (int b = 0; b < batch; ++b) CHECK(owners[b] == 1, "batch %d tiles %lld nb %d: frame set %d has %d blocks", batch, tiles, nb, b, owners[b]);
            // the heuristic's own statement: the largest nb <= 16 that leaves kMovingMinBlocks blocks, or 1
            CHECK(nb == 1 || tiles * blocks >= kMovingMinBlocks, "batch %d tiles %lld nb %d: %lld blocks", batch, tiles, nb, tiles * blocks);
            CHECK(nb == 16 || tiles * ((batch + 2 * nb - 1) / (2 * nb)) < kMovingMinBlocks, "batch %d tiles %lld: nb %d could be doubled", batch, tiles, nb);
            ++cases;
        }
    printf("moving blocks ok: %llu cases\n", cases);
    return 0;
}

static int units_census(const char *path)
{
    FILE *f = fopen(path, "rb");
    CHECK(f, "cannot read %s", path);
    int32_t head[4];
    CHECK(fread(head, 4, 4, f) == 4, "short header");
    const int fw = head[0], fh = head[1], bw = head[2], bh = head[3];
    CHECK(fw > 0 && fh > 0 && bw > 0 && bh > 0 && fw % 4 == 0 && bw % 4 == 0, "bad header");
    const size_t npx = (size_t)bw * bh;
    std::vector<int16_t> m1(npx * 2);
    std::vector<uint16_t> m2(npx);
    CHECK(fread(m1.data(), 2, npx * 2, f) == npx * 2 && fread(m2.data(), 2, npx, f) == npx, "short input");
    fclose(f);
    const int tiles_x = (bw + 31) / 32, tiles_y = (bh + 7) / 8;
    std::vector<int16_t> l1[4] = {m1};
    std::vector<uint16_t> l2[4] = {m2};
    std::vector<uint8_t> mk[4] = {std::vector<uint8_t>(npx, 255)};
    std::vector<uint32_t> hdr = unit_host_headers(l1, mk, 1, fw, fh, bw, bh, tiles_x, tiles_y);
    UnitPlanHost up;
    UnitTuning tune;
    tune.row_order = 4;   // as plan_build orders a one-camera plan
    unit_compile(l1, l2, mk, 1, fw, fh, bw, bh, bw, tiles_x, tiles_y, hdr, up, tune);
    size_t empty = 0;
    for (const UnitDesc &d : up.desc) empty += d.groups == 0;
    const size_t tiles = (size_t)tiles_x * tiles_y;
    CHECK(up.claimed_tiles <= tiles, "claimed %zu of %zu tiles", up.claimed_tiles, tiles);
    printf("units %zu empty %zu tiles %zu per_tap %zu\n", up.desc.size(), empty, tiles, tiles - up.claimed_tiles);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "--bevw-selfcheck-noop") == 0) return 0;
    if (argc == 2 && strcmp(argv[1], "--moving-nb") == 0) return moving_enumerate();
    if (argc >= 4 && strcmp(argv[1], "--moving-table") == 0) {
        const long long tiles = atoll(argv[2]);
        CHECK(tiles >= 1, "tiles '%s'", argv[2]);
        for (int i = 3; i < argc; ++i) {
            const int batch = atoi(argv[i]);
            CHECK(batch >= 1, "batch '%s'", argv[i]);
            const int nb = moving_nb(batch, tiles), blocks = (batch + nb - 1) / nb;
            printf("%d %d %d %d\n", batch, nb, blocks, batch - (blocks - 1) * nb);
        }
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "--units") == 0) return units_census(argv[2]);
    CHECK(false, "usage: batch_loops_census --moving-nb | --moving-table TILES B ... | --units <in>");
}
