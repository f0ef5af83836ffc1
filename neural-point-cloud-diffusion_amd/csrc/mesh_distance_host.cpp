// The launches of mesh_distance.hip on the host: the per-lane functions of mesh_distance.h, the code the kernels run, as plain loops
// over faces, tiles and query points.  A stand-alone program for tests/test_mesh_distance_cpu.py, which holds its output to
// npcd.eval.mesh.point_mesh_distance_reference before the kernels run anywhere; it is not part of libnpcd_hip.so.
//
//   mesh_distance_host IN OUT [reverse]
//   IN:  int32 S, V, F; float32 points [S, 3], vertices [V, 3]; int32 faces [F, 3]
//   OUT: twice (every face through the packed-key minimum, then the culled walk of the kernel with a wave of one lane):
//        float32 sqdist [S]; int32 face [S]; float32 closest [S, 3];
//        then int64 violations, evaluated, pairs: the (point, face) pairs with a dist2 that can win, below +inf, whose tile a lane
//        with that dist2 as its best would skip (md_needs of the tile's bound); the tiles the culled walk evaluated; S times the tiles.
// With `reverse` the faces of the first pass and the tiles of the culled walk are visited in descending order: a lexicographic minimum
// does not depend on the schedule.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_lanes.h"
#include "mesh_distance.h"

using namespace npcd;

struct Result {
    std::vector<float> sqdist, closest;
    std::vector<int32_t> face;
    explicit Result(int64_t S) : sqdist(S, -7.f), closest((size_t)S * 3, -7.f), face(S, -7) {}
};

static float pair_of(const float* p, const std::vector<MdCorner>& corners, int64_t f, float* q) {
    const MdCorner* c = corners.data() + f * 3;
    const float a[3] = {c[0].x, c[0].y, c[0].z}, b[3] = {c[1].x, c[1].y, c[1].z}, cc[3] = {c[2].x, c[2].y, c[2].z};
    return md_pair(p, a, b, cc, q);
}

// what the kernel stores for a point whose winner is (best, best_face)
static void finish(const float* p, const std::vector<MdCorner>& corners, float best, int32_t best_face, int64_t i, Result& out) {
    float q[3] = {0.f, 0.f, 0.f};
    if (best_face >= 0) pair_of(p, corners, best_face, q);
    out.sqdist[i] = best, out.face[i] = best_face;
    for (int k = 0; k < 3; ++k) out.closest[i * 3 + k] = q[k];
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool reverse = argc > 3 && !std::strcmp(argv[3], "reverse");
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[3];
    if (std::fread(head, 4, 3, in) != 3) return 2;
    const int64_t S = head[0], V = head[1], F = head[2];
    if (S < 0 || V < 0 || F < 0 || F >= kMdMaxFaces) return 2;
    std::vector<float> points((size_t)S * 3), vertices((size_t)V * 3);
    std::vector<int32_t> faces((size_t)F * 3);
    if (!read_all(in, points) || !read_all(in, vertices) || !read_all(in, faces)) return 2;
    std::fclose(in);
    const int64_t tiles = md_tiles(F);
    const LaneOrder order{reverse};
    // ---- the boxes launch ----------------------------------------------------------------------------------------------------------------
    const MdCorner poison = {-7.f, -7.f, -7.f, -7.f};
    std::vector<MdCorner> corners((size_t)tiles * kMdTile * 3, poison);
    std::vector<MdBox> boxes(tiles);
    for (int64_t l = 0; l < tiles * kMdTile; ++l) {
        const int64_t f = order(l, tiles * kMdTile);
        md_corners_lane(vertices.data(), V, faces.data(), F, f, corners.data() + f * 3);
    }
    for (int64_t t = 0; t < tiles; ++t) boxes[t] = md_box_of(corners.data() + t * kMdTile * 3, kMdTile * 3);
    // ---- every face, through the packed key ----------------------------------------------------------------------------------------------
    Result all(S), culled(S);
    int64_t violations = 0, evaluated = 0;
    std::vector<float> bound(tiles);
    for (int64_t i = 0; i < S; ++i) {
        const float* p = points.data() + i * 3;
        const float point_slack = md_point_slack(p);
        for (int64_t t = 0; t < tiles; ++t) bound[t] = md_bound(p, point_slack, boxes[t]);
        uint64_t best = kMdNoKey;
        for (int64_t l = 0; l < F; ++l) {
            const int64_t f = order(l, F);
            float q[3];
            const float d = pair_of(p, corners, f, q);
            const uint64_t key = md_key(d, (int32_t)f);
            best = key < best ? key : best;
            const float b = bound[f / kMdTile];
            if (key != kMdNoKey && !md_needs(b, d)) violations += 1;          // a face that can win, in a tile that a lane with this best skips
        }
        finish(p, corners, bits_float((uint32_t)(best >> 32)), (int32_t)(uint32_t)best, i, all);
    }
    // ---- the culled walk of the kernel, a wave of one lane ---------------------------------------------------------------------------------
    for (int64_t i = 0; i < S; ++i) {
        const float* p = points.data() + i * 3;
        const float point_slack = md_point_slack(p);
        float best = bits_float(kMdInfBits), least = best;
        int32_t best_face = -1;
        int64_t nearest = -1;
        const auto evaluate = [&](int64_t t) {
            for (int64_t f = t * kMdTile; f < F && f < (t + 1) * kMdTile; ++f) {
                float q[3];
                const float d = pair_of(p, corners, f, q);
                if (md_better(d, (int32_t)f, best, best_face)) best = d, best_face = (int32_t)f;
            }
            evaluated += 1;
        };
        for (int64_t t = 0; t < tiles; ++t) {
            const float b = md_bound(p, point_slack, boxes[t]);
            if (b < least) least = b, nearest = t;
        }
        if (nearest >= 0) evaluate(nearest);
        for (int64_t l = 0; l < tiles; ++l) {
            const int64_t t = order(l, tiles);
            if (t == nearest) continue;
            if (md_needs(md_bound(p, point_slack, boxes[t]), best)) evaluate(t);
        }
        finish(p, corners, best, best_face, i, culled);
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    const int64_t tail[3] = {violations, evaluated, S * tiles};
    const bool ok = write_all(fo, all.sqdist) && write_all(fo, all.face) && write_all(fo, all.closest) && write_all(fo, culled.sqdist) &&
                    write_all(fo, culled.face) && write_all(fo, culled.closest) && std::fwrite(tail, 8, 3, fo) == 3;
    return std::fclose(fo) == 0 && ok ? 0 : 2;
}
