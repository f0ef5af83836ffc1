// The labelling phases of components.h on the host: the functions the kernels of components.hip run, as plain loops over workgroups
// and lanes with plain memory operations.  A stand-alone program for tests/test_components_cpu.py, which holds its output to
// npcd.eval.mesh.connected_components_reference before the kernels run anywhere; it is not part of libnpcd_hip.so.
//
//   components_host IN OUT [reverse]
//   IN:  int32 B, gz, gy, gx; float32 level; float32 vol [B, gz, gy, gx]
//   OUT: int32 labels [B, n]; int32 sizes [B, n]
// With `reverse` the workgroups and the lanes of every step run in descending order: the result does not depend on the schedule.
#include <cstdio>
#include <cstring>
#include <vector>

#include "components.h"
#include "host_lanes.h"

using namespace npcd;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool reverse = argc > 3 && !std::strcmp(argv[3], "reverse");
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t dims[4];
    float level;
    if (std::fread(dims, 4, 4, in) != 4 || std::fread(&level, 4, 1, in) != 1) return 2;
    const int B = dims[0];
    if (B < 1 || dims[1] < 2 || dims[2] < 2 || dims[3] < 2 || (int64_t)dims[1] * dims[2] * dims[3] >= (int64_t)1 << 31) return 2;
    const CcGrid g = cc_grid(dims[1], dims[2], dims[3]);
    std::vector<float> vol((size_t)B * g.n);
    if (std::fread(vol.data(), 4, vol.size(), in) != vol.size()) return 2;
    std::fclose(in);
    // poisoned: the phases write every entry they promise
    std::vector<int32_t> parent(vol.size(), -7), labels(vol.size(), -7), sizes(vol.size(), -7);
    const LaneOrder order{reverse};
    for (int b = 0; b < B; ++b) {
        const size_t base = (size_t)b * g.n;
        for (int w = 0; w < g.bricks; ++w) {          // tile phase: one workgroup per brick, a barrier between the steps
            const int brick = order(w, g.bricks);
            int32_t local[kCcBrickNodes], count[kCcBrickNodes];
            for (int i = 0; i < kCcBrickNodes; ++i) cc_tile_load(g, vol.data() + base, level, brick, order(i, kCcBrickNodes), local, count);
            for (int i = 0; i < kCcBrickNodes; ++i) cc_tile_link<CcPlain>(order(i, kCcBrickNodes), local);
            for (int i = 0; i < kCcBrickNodes; ++i) cc_tile_count<CcPlain>(order(i, kCcBrickNodes), local, count);
            for (int i = 0; i < kCcBrickNodes; ++i)
                cc_tile_store(g, brick, order(i, kCcBrickNodes), local, count, parent.data() + base, sizes.data() + base);
        }
        for (int w = 0; w < g.bricks; ++w)          // merge phase
            for (int i = 0; i < kCcBrickNodes; ++i)
                cc_merge_node<CcPlain>(g, order(w, g.bricks), order(i, kCcBrickNodes), parent.data() + base);
        for (int i = 0; i < g.n; ++i)          // final phase
            cc_final_node<CcPlain>(parent.data() + base, order(i, g.n), labels.data() + base, sizes.data() + base);
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = std::fwrite(labels.data(), 4, labels.size(), out) == labels.size() &&
                    std::fwrite(sizes.data(), 4, sizes.size(), out) == sizes.size();
    return std::fclose(out) == 0 && ok ? 0 : 2;
}
