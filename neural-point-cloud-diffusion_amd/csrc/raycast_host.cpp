// The launch of raycast.hip on the host: the per-lane functions of raycast.h, the code the kernel runs, as plain loops over faces,
// tiles and rays, on the corners and boxes that the functions of mesh_distance.h leave.  A stand-alone program for
// tests/test_raycast_cpu.py, which holds its output to npcd.eval.mesh.ray_mesh_reference before the kernel runs anywhere; it is not
// part of libnpcd_hip.so.
//
//   raycast_host IN OUT [reverse]
//   IN:  int32 R, V, F; float32 t_min, t_max; float32 origins [R, 3], directions [R, 3], vertices [V, 3]; int32 faces [F, 3]
//   OUT: twice (every face through the packed-key minimum, then the culled walk of the kernel with a wave of one lane):
//        float32 t [R]; int32 face [R]; float32 bary [R, 3]; int8 front [R];
//        then int64 violations, evaluated, pairs: the (ray, face) hits whose tile a lane with that t as its best would skip
//        (rc_reach of the tile's box); the tiles the culled walk evaluated; R times the tiles.
// With `reverse` the faces of the first pass and the tiles of the culled walk are visited in descending order: a lexicographic minimum
// does not depend on the schedule.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_lanes.h"
#include "raycast.h"

using namespace npcd;

struct Result {
    std::vector<float> t, bary;
    std::vector<int32_t> face;
    std::vector<int8_t> front;
    explicit Result(int64_t R) : t(R, -7.f), bary((size_t)R * 3, -7.f), face(R, -7), front(R, -7) {}
};

static RcPair pair_of(const RcRay& ray, const std::vector<MdCorner>& corners, int64_t f) {
    const MdCorner* c = corners.data() + f * 3;
    const float a[3] = {c[0].x, c[0].y, c[0].z}, b[3] = {c[1].x, c[1].y, c[1].z}, cc[3] = {c[2].x, c[2].y, c[2].z};
    return rc_pair(ray, a, b, cc);
}

// what the kernel stores for a ray whose winner is best_face
static void finish(const RcRay& ray, const std::vector<MdCorner>& corners, int32_t best_face, int64_t i, Result& out) {
    float t = bits_float(kMdInfBits), bary[3] = {0.f, 0.f, 0.f};
    int8_t front = 0;
    if (best_face >= 0) {
        const RcPair p = pair_of(ray, corners, best_face);
        t = p.t;
        rc_finish(p, bary, &front);
    }
    out.t[i] = t, out.face[i] = best_face, out.front[i] = front;
    for (int k = 0; k < 3; ++k) out.bary[i * 3 + k] = bary[k];
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool reverse = argc > 3 && !std::strcmp(argv[3], "reverse");
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[3];
    float limits[2];
    if (std::fread(head, 4, 3, in) != 3 || std::fread(limits, 4, 2, in) != 2) return 2;
    const int64_t R = head[0], V = head[1], F = head[2];
    const float t_min = limits[0], t_max = limits[1];
    if (R < 0 || V < 0 || F < 0 || F >= kMdMaxFaces) return 2;
    std::vector<float> origins((size_t)R * 3), directions((size_t)R * 3), vertices((size_t)V * 3);
    std::vector<int32_t> faces((size_t)F * 3);
    if (!read_all(in, origins) || !read_all(in, directions) || !read_all(in, vertices) || !read_all(in, faces)) return 2;
    std::fclose(in);
    const int64_t tiles = md_tiles(F);
    const LaneOrder order{reverse};
    // ---- the boxes launch of mesh_distance.hip ---------------------------------------------------------------------------------------------
    const MdCorner poison = {-7.f, -7.f, -7.f, -7.f};
    std::vector<MdCorner> corners((size_t)tiles * kMdTile * 3, poison);
    std::vector<MdBox> boxes(tiles);
    for (int64_t f = 0; f < tiles * kMdTile; ++f) md_corners_lane(vertices.data(), V, faces.data(), F, f, corners.data() + f * 3);
    for (int64_t t = 0; t < tiles; ++t) boxes[t] = md_box_of(corners.data() + t * kMdTile * 3, kMdTile * 3);
    // ---- every face, through the packed key ----------------------------------------------------------------------------------------------
    Result all(R), culled(R);
    int64_t violations = 0, evaluated = 0;
    for (int64_t i = 0; i < R; ++i) {
        const RcRay ray = rc_ray(origins.data() + i * 3, directions.data() + i * 3);
        uint64_t best = kRcNoKey;
        for (int64_t l = 0; l < F; ++l) {
            const int64_t f = order(l, F);
            const RcPair p = pair_of(ray, corners, f);
            if (!p.inside || !rc_hit(p.t, t_min, t_max)) continue;
            const uint64_t key = rc_key(p.t, (int32_t)f);
            best = key < best ? key : best;
            float enter;
            const float to = p.t < t_max ? p.t : t_max;
            if (!rc_reach(ray, boxes[f / kMdTile], t_min, to, &enter)) violations += 1;          // a hit in a tile that a lane with this best skips
        }
        finish(ray, corners, best == kRcNoKey ? -1 : (int32_t)(uint32_t)best, i, all);
    }
    // ---- the culled walk of the kernel, a wave of one lane ---------------------------------------------------------------------------------
    for (int64_t i = 0; i < R; ++i) {
        const RcRay ray = rc_ray(origins.data() + i * 3, directions.data() + i * 3);
        const float inf = bits_float(kMdInfBits);
        float best = inf, least = inf;
        int32_t best_face = -1;
        int64_t nearest = -1;
        const auto evaluate = [&](int64_t t) {
            for (int64_t f = t * kMdTile; f < F && f < (t + 1) * kMdTile; ++f) {
                const RcPair p = pair_of(ray, corners, f);
                if (p.inside && rc_hit(p.t, t_min, t_max) && rc_better(p.t, (int32_t)f, best, best_face)) best = p.t, best_face = (int32_t)f;
            }
            evaluated += 1;
        };
        for (int64_t t = 0; t < tiles; ++t) {
            float enter;
            if (rc_reach(ray, boxes[t], t_min, t_max, &enter) && enter < least) least = enter, nearest = t;
        }
        if (nearest >= 0) evaluate(nearest);
        for (int64_t l = 0; l < tiles; ++l) {
            const int64_t t = order(l, tiles);
            if (t == nearest) continue;
            float enter;
            if (rc_reach(ray, boxes[t], t_min, best < t_max ? best : t_max, &enter)) evaluate(t);
        }
        finish(ray, corners, best_face, i, culled);
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    const int64_t tail[3] = {violations, evaluated, R * tiles};
    bool ok = true;
    for (const Result* r : {&all, &culled}) ok = ok && write_all(fo, r->t) && write_all(fo, r->face) && write_all(fo, r->bary) && write_all(fo, r->front);
    ok = ok && std::fwrite(tail, 8, 3, fo) == 3;
    return std::fclose(fo) == 0 && ok ? 0 : 2;
}
