// The launches of mesh_distance.hip on the host: the per-lane functions of mesh_tiles.h and mesh_distance.h and the MdQuery policy, the
// code the kernels run, under the host's tile walk (host_lanes.h).  A stand-alone program for tests/test_mesh_distance_cpu.py, which
// holds its output to npcd.eval.mesh.point_mesh_distance_reference before the kernels run anywhere; it is not part of libnpcd_hip.so.
//
//   mesh_distance_host IN OUT [reverse] [wave]
//   IN:  int32 S, V, F; float32 points [S, 3], vertices [V, 3]; int32 faces [F, 3]
//   OUT: twice (every face through the packed-key minimum, then the culled walk of the kernel in waves of one lane, with `wave` of
//        kMdThreads consecutive points):
//        float32 sqdist [S]; int32 face [S]; float32 closest [S, 3];
//        then int64 violations, evaluated, pairs: the (point, face) pairs with a dist2 that can win, below +inf, whose tile a lane
//        with that dist2 as its best would skip (md_needs of the tile's bound); the (wave, tile) pairs the culled walk evaluated; the
//        waves times the tiles.
// With `reverse` the faces of the first pass and the tiles of the culled walk are visited in descending order.
#include <cstring>

#include "host_lanes.h"
#include "mesh_distance.h"

using namespace npcd;

struct Result {
    std::vector<float> sqdist, closest;
    std::vector<int32_t> face;
    explicit Result(int64_t S) : sqdist(S, -7.f), closest((size_t)S * 3, -7.f), face(S, -7) {}
    bool write(FILE* fo) const { return write_all(fo, sqdist) && write_all(fo, face) && write_all(fo, closest); }
};

// what the kernel stores for a point whose winner is (best, best_face)
static void finish(const MdQuery& query, const HostTiles& m, float best, int32_t best_face, int64_t i, Result& out) {
    float q[3] = {0.f, 0.f, 0.f};
    if (best_face >= 0) query.pair(m.face(best_face), q);
    out.sqdist[i] = best, out.face[i] = best_face;
    for (int k = 0; k < 3; ++k) out.closest[i * 3 + k] = q[k];
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    int64_t S, V, F;
    if (!in || !read_head(in, &S, &V, &F)) return 2;
    std::vector<float> points((size_t)S * 3), vertices((size_t)V * 3);
    std::vector<int32_t> faces((size_t)F * 3);
    if (!read_all(in, points) || !read_all(in, vertices) || !read_all(in, faces)) return 2;
    std::fclose(in);
    const LaneOrder order{argc > 3 && !std::strcmp(argv[3], "reverse")};
    const HostTiles m(vertices, V, faces, F, order);
    std::vector<MdQuery> queries;
    for (int64_t i = 0; i < S; ++i) queries.push_back(md_query(points.data() + i * 3, true));
    // ---- every face, through the packed key ----------------------------------------------------------------------------------------------
    Result all(S), culled(S);
    int64_t violations = 0;
    std::vector<float> bound(m.tiles);
    for (int64_t i = 0; i < S; ++i) {
        const MdQuery& query = queries[i];
        for (int64_t t = 0; t < m.tiles; ++t) bound[t] = md_bound(query.p, query.slack, m.boxes[t]);
        uint64_t best = kMdNoKey;
        for (int64_t l = 0; l < F; ++l) {
            const int64_t f = order(l, F);
            float q[3];
            const float d = query.pair(m.face(f), q);
            const uint64_t key = md_key(d, (int32_t)f);
            best = key < best ? key : best;
            if (key != kMdNoKey && !md_needs(bound[f / kMdTile], d)) violations += 1;          // a face that can win, in a tile that a lane with this best skips
        }
        finish(query, m, bits_float((uint32_t)(best >> 32)), (int32_t)(uint32_t)best, i, all);
    }
    // ---- the culled walk of the kernel ---------------------------------------------------------------------------------------------------
    const int W = argc > 3 && !std::strcmp(argv[argc - 1], "wave") ? kMdThreads : 1;
    const auto store = [&](int64_t i, float best, int32_t best_face) { finish(queries[i], m, best, best_face, i, culled); };
    const int64_t evaluated = W == 1 ? host_tile_walk<MdQuery, 1>(queries, m, order, store) : host_tile_walk<MdQuery, kMdThreads>(queries, m, order, store);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    return write_tail(fo, all.write(fo) && culled.write(fo), violations, evaluated, (S + W - 1) / W * m.tiles);
}
