// The launch of raycast.hip on the host: the per-lane functions of raycast.h and the RcQuery policy, the code the kernel runs, under
// the host's tile walk (host_lanes.h), on the corners and boxes that the functions of mesh_tiles.h leave.  A stand-alone program
// for tests/test_raycast_cpu.py, which holds its output to npcd.eval.mesh.ray_mesh_reference before the kernel runs anywhere; it is
// not part of libnpcd_hip.so.
//
//   raycast_host IN OUT [reverse] [wave]
//   IN:  int32 R, V, F; float32 t_min, t_max; float32 origins [R, 3], directions [R, 3], vertices [V, 3]; int32 faces [F, 3]
//   OUT: twice (every face through the packed-key minimum, then the culled walk of the kernel in waves of one lane, with `wave` of
//        kRcThreads consecutive rays):
//        float32 t [R]; int32 face [R]; float32 bary [R, 3]; int8 front [R];
//        then int64 violations, evaluated, pairs: the (ray, face) hits whose tile a lane with that t as its best would skip
//        (rc_reach of the tile's box); the (wave, tile) pairs the culled walk evaluated; the waves times the tiles.
// With `reverse` the faces of the first pass and the tiles of the culled walk are visited in descending order.
#include <cstring>

#include "host_lanes.h"
#include "raycast.h"

using namespace npcd;

struct Result {
    std::vector<float> t, bary;
    std::vector<int32_t> face;
    std::vector<int8_t> front;
    explicit Result(int64_t R) : t(R, -7.f), bary((size_t)R * 3, -7.f), face(R, -7), front(R, -7) {}
    bool write(FILE* fo) const { return write_all(fo, t) && write_all(fo, face) && write_all(fo, bary) && write_all(fo, front); }
};

// what the kernel stores for a ray whose winner is best_face
static void finish(const RcQuery& query, const HostTiles& m, int32_t best_face, int64_t i, Result& out) {
    float t = bits_float(kMdInfBits), bary[3] = {0.f, 0.f, 0.f};
    int8_t front = 0;
    if (best_face >= 0) {
        const RcPair p = query.pair(m.face(best_face));
        t = p.t;
        rc_finish(p, bary, &front);
    }
    out.t[i] = t, out.face[i] = best_face, out.front[i] = front;
    for (int k = 0; k < 3; ++k) out.bary[i * 3 + k] = bary[k];
}

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
    std::vector<RcQuery> queries;
    for (int64_t i = 0; i < R; ++i) queries.push_back(RcQuery{rc_ray(origins.data() + i * 3, directions.data() + i * 3), t_min, t_max});
    // ---- every face, through the packed key ----------------------------------------------------------------------------------------------
    Result all(R), culled(R);
    int64_t violations = 0;
    for (int64_t i = 0; i < R; ++i) {
        uint64_t best = kRcNoKey;
        for (int64_t l = 0; l < F; ++l) {
            const int64_t f = order(l, F);
            const RcPair p = queries[i].pair(m.face(f));
            if (!p.inside || !rc_hit(p.t, t_min, t_max)) continue;
            const uint64_t key = rc_key(p.t, (int32_t)f);
            best = key < best ? key : best;
            if (!queries[i].recall(m.boxes[f / kMdTile], p.t)) violations += 1;          // a hit in a tile that a lane with this best skips
        }
        finish(queries[i], m, best == kRcNoKey ? -1 : (int32_t)(uint32_t)best, i, all);
    }
    // ---- the culled walk of the kernel ---------------------------------------------------------------------------------------------------
    const int W = argc > 3 && !std::strcmp(argv[argc - 1], "wave") ? kRcThreads : 1;
    const auto store = [&](int64_t i, float, int32_t best_face) { finish(queries[i], m, best_face, i, culled); };
    const int64_t evaluated = W == 1 ? host_tile_walk<RcQuery, 1>(queries, m, order, store) : host_tile_walk<RcQuery, kRcThreads>(queries, m, order, store);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    return write_tail(fo, all.write(fo) && culled.write(fo), violations, evaluated, (R + W - 1) / W * m.tiles);
}
