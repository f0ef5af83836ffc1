// The launch of crossings.hip on the host: the per-lane functions of raycast.h and the CrQuery policy, the code the kernel runs, under
// the host's tile sweep (host_lanes.h), on the corners and boxes that the functions of mesh_tiles.h leave.  A stand-alone program
// for tests/test_crossings_cpu.py, which holds its output to npcd.eval.mesh.crossings_reference before the kernel runs anywhere; it
// is not part of libnpcd_hip.so.
//
//   crossings_host IN OUT [reverse] [wave]
//   IN:  int32 R, V, F; float32 t_min, t_max; float32 origins [R, 3], directions [R, 3], vertices [V, 3]; int32 faces [F, 3]
//   OUT: twice (every face, then the culled sweep of the kernel in waves of one lane, with `wave` of kRcThreads consecutive rays):
//        int32 front [R]; int32 back [R];
//        then int64 violations, evaluated, pairs: the counted (ray, face) crossings whose tile the ray does not reach (rc_reach of
//        the tile's box); the (wave, tile) pairs the culled sweep evaluated; the waves times the tiles.
// With `reverse` the faces of the first pass and the tiles of the culled sweep are visited in descending order.
#include <cstring>

#include "host_lanes.h"
#include "raycast.h"

using namespace npcd;

struct Result {
    std::vector<int32_t> front, back;
    explicit Result(int64_t R) : front(R, -7), back(R, -7) {}
    void store(int64_t i, const RcCrossings& count) { front[i] = count.front, back[i] = count.back; }
    bool write(FILE* fo) const { return write_all(fo, front) && write_all(fo, back); }
};

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    int64_t R, V, F;
    float limits[2];
    if (!in || !read_head(in, &R, &V, &F) || std::fread(limits, 4, 2, in) != 2) return 2;
    const float t_min = limits[0], t_max = limits[1];
    std::vector<float> origins((size_t)R * 3), directions((size_t)R * 3), vertices((size_t)V * 3);
    std::vector<int32_t> faces((size_t)F * 3);
    if (!read_all(in, origins) || !read_all(in, directions) || !read_all(in, vertices) || !read_all(in, faces)) return 2;
    std::fclose(in);
    const LaneOrder order{argc > 3 && !std::strcmp(argv[3], "reverse")};
    const HostTiles m(vertices, V, faces, F, order);
    std::vector<CrQuery> queries;
    for (int64_t i = 0; i < R; ++i) queries.push_back(CrQuery{rc_ray(origins.data() + i * 3, directions.data() + i * 3), t_min, t_max});
    // ---- every face ------------------------------------------------------------------------------------------------------------------------
    Result all(R), culled(R);
    int64_t violations = 0;
    for (int64_t i = 0; i < R; ++i) {
        RcCrossings count{0, 0};
        for (int64_t l = 0; l < F; ++l) {
            const int64_t f = order(l, F);
            const RcCrossings before = count;
            queries[i].face(m.face(f), (int32_t)f, &count);
            const bool counted = count.front != before.front || count.back != before.back;
            if (counted && !queries[i].reaches(m.boxes[f / kMdTile])) violations += 1;          // a crossing in a tile that the lane skips
        }
        all.store(i, count);
    }
    // ---- the culled sweep of the kernel --------------------------------------------------------------------------------------------------
    const int W = argc > 3 && !std::strcmp(argv[argc - 1], "wave") ? kRcThreads : 1;
    const auto store = [&](int64_t i, const RcCrossings& count) { culled.store(i, count); };
    const int64_t evaluated = W == 1 ? host_tile_sweep<CrQuery, 1>(queries, m, order, store) : host_tile_sweep<CrQuery, kRcThreads>(queries, m, order, store);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    return write_tail(fo, all.write(fo) && culled.write(fo), violations, evaluated, (R + W - 1) / W * m.tiles);
}
