// The closest point of a triangle mesh to a query point: the per-lane arithmetic of csrc/mesh_distance.hip, written
// once for the device and the host.  The kernels run these functions and those of mesh_tiles.h one lane per face (the corners launch) or per query
// point; the stand-alone program csrc/mesh_distance_host.cpp runs them as plain loops (tests/test_mesh_distance_cpu.py): this header
// includes nothing of HIP.  All fp32 arithmetic is as written -- the file is compiled without FMA contraction (build.py) -- and the division
// is the correctly rounded one.
//
//   Pair      (p; a, b, c): the region form of Ericson's closest point on a triangle, md_pair below; dot(u, v) = (ux vx + uy vy) +
//             uz vz.  The first region that holds gives (v, w); q = a + (v ab + w ac), dist2 = dot(p - q, p - q).  One division: the
//             regions differ in which quotient they take, not in how it is rounded.
//   Winner    the lexicographic minimum of (dist2, face) over the faces with dist2 < +inf; a NaN never wins.  dist2 >= +0, so its
//             bits order as unsigned integers: md_key packs (bits << 32) | face.
//   Bound     md_bound: g = (max(lo - p, p - hi) - max(slack, the point's own)) (1 - 2^-11), clamped at 0 per axis; (gx gx + gy gy) +
//             gz gz.  A tile is evaluated if bound <= best and bound < +inf (md_needs); the box of a tile without a finite corner
//             is (+inf, -inf), whose bound is +inf for every finite point.
//   Query     MdQuery: a lane's point and slack, and the answers of these functions to the tile walk (tile_walk.h).
#pragma once
#include <math.h>
#include <stdint.h>

#include "bits.h"
#include "mesh_tiles.h"

namespace npcd {

constexpr int kMdThreads = 64;                                // lanes per workgroup of the query launch: one wave, one point per lane
constexpr int kMdScan = 4;                                    // boxes a wave takes bounds to at a time: their loads are in flight together
constexpr int64_t kMdMaxPoints = (int64_t)1 << 31;
constexpr uint64_t kMdNoKey = ((uint64_t)kMdInfBits << 32) | 0xffffffffu;          // (+inf, -1): what a point without a face keeps
constexpr float kMdShrink = 0.99951171875f;                   // 1 - 2^-11, per axis: 2^-10 of the bound

NPCD_HD float md_dot(float ux, float uy, float uz, float vx, float vy, float vz) { return (ux * vx + uy * vy) + uz * vz; }

// ---- one pair -------------------------------------------------------------------------------------------------------------------------
// -> dist2; q [3] the closest point
NPCD_HD float md_pair(const float* p, const float* a, const float* b, const float* c, float* q) {
    const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
    const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
    const float apx = p[0] - a[0], apy = p[1] - a[1], apz = p[2] - a[2];
    const float bpx = p[0] - b[0], bpy = p[1] - b[1], bpz = p[2] - b[2];
    const float cpx = p[0] - c[0], cpy = p[1] - c[1], cpz = p[2] - c[2];
    const float d1 = md_dot(abx, aby, abz, apx, apy, apz), d2 = md_dot(acx, acy, acz, apx, apy, apz);
    const float d3 = md_dot(abx, aby, abz, bpx, bpy, bpz), d4 = md_dot(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = md_dot(abx, aby, abz, cpx, cpy, cpz), d6 = md_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    // no short-circuit anywhere below: the lanes of a wave fall into different regions, and selects cost less than branches
    const bool at_a = (d1 <= 0.f) & (d2 <= 0.f);
    const bool at_b = (d3 >= 0.f) & (d4 <= d3);
    const bool on_ab = (vc <= 0.f) & (d1 >= 0.f) & (d3 <= 0.f);
    const bool at_c = (d6 >= 0.f) & (d5 <= d6);
    const bool on_ac = (vb <= 0.f) & (d2 >= 0.f) & (d6 <= 0.f);
    const bool on_bc = (va <= 0.f) & (d43 >= 0.f) & (d56 >= 0.f);
    // the first region that holds: a, b, ab, c, ac, bc, inside
    const bool is_b = !at_a & at_b, none2 = !at_a & !at_b;
    const bool is_ab = none2 & on_ab, none3 = none2 & !on_ab;
    const bool is_c = none3 & at_c, none4 = none3 & !at_c;
    const bool is_ac = none4 & on_ac, none5 = none4 & !on_ac;
    const bool is_bc = none5 & on_bc, inside = none5 & !on_bc;
    float num = 1.f, den = (va + vb) + vc;
    num = is_ab ? d1 : num, den = is_ab ? d1 - d3 : den;
    num = is_ac ? d2 : num, den = is_ac ? d2 - d6 : den;
    num = is_bc ? d43 : num, den = is_bc ? d43 + d56 : den;
    const float r = num / den;          // not used by the corner regions, whatever it is
    float v = 0.f, w = 0.f;
    v = is_b ? 1.f : v;
    v = is_ab ? r : v;
    w = is_c ? 1.f : w;
    w = is_ac ? r : w;
    v = is_bc ? 1.f - r : v, w = is_bc ? r : w;
    v = inside ? vb * r : v, w = inside ? vc * r : w;
    q[0] = a[0] + (v * abx + w * acx), q[1] = a[1] + (v * aby + w * acy), q[2] = a[2] + (v * abz + w * acz);
    const float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
    return md_dot(ex, ey, ez, ex, ey, ez);
}

// ---- the winner -----------------------------------------------------------------------------------------------------------------------
// (dist2, face) replaces (best, best_face) if it is below it lexicographically; a NaN and +inf never do
NPCD_HD bool md_better(float dist2, int32_t face, float best, int32_t best_face) {
    return (dist2 < best) | ((dist2 == best) & (face < best_face));
}
// the same order on one word: a dist2 that cannot win (NaN, +inf) gives kMdNoKey
NPCD_HD uint64_t md_key(float dist2, int32_t face) {
    return dist2 < bits_float(kMdInfBits) ? ((uint64_t)float_bits(dist2) << 32) | (uint32_t)face : kMdNoKey;
}

// ---- one (point, tile) of the query launch ----------------------------------------------------------------------------------------------
NPCD_HD float md_bound(const float* p, float point_slack, const MdBox& box) {
    const float slack = box.slack > point_slack ? box.slack : point_slack;
    float g[3];
    for (int k = 0; k < 3; ++k) {
        const float below = box.lo[k] - p[k], above = p[k] - box.hi[k];
        const float out = ((below > above ? below : above) - slack) * kMdShrink;
        g[k] = out > 0.f ? out : 0.f;          // a NaN gives 0
    }
    return md_dot(g[0], g[1], g[2], g[0], g[1], g[2]);
}
NPCD_HD bool md_needs(float bound, float best) { return !(bound > best) & (bound < bits_float(kMdInfBits)); }

// ---- what the tile walk asks of a point (tile_walk.h on the device, host_lanes.h on the host) -----------------------
struct MdQuery {
    static constexpr int kLanes = kMdThreads, kScan = kMdScan;
    typedef TileWinner State;
    typedef float Memo;          // the bound to a box: it does not depend on best, md_needs sees the best of the moment
    float p[3], slack;
    bool own;                    // the lane holds a point: one that does not ranks no box and needs no tile
    NPCD_HD bool rank(const MdBox& box, float* value) const { return *value = md_bound(p, slack, box), own; }
    NPCD_HD Memo recall(const MdBox& box, float) const { return md_bound(p, slack, box); }
    NPCD_HD bool needs(Memo bound, float best) const { return own & md_needs(bound, best); }
    // -> dist2 to the face of corners c [3]; q [3] the closest point
    NPCD_HD float pair(const MdCorner* c, float* q) const {
        const float fa[3] = {c[0].x, c[0].y, c[0].z}, fb[3] = {c[1].x, c[1].y, c[1].z}, fc[3] = {c[2].x, c[2].y, c[2].z};
        return md_pair(p, fa, fb, fc, q);
    }
    NPCD_HD void face(const MdCorner* c, int32_t f, State* won) const {
        float q[3];
        const float d = pair(c, q);
        const bool better = md_better(d, f, won->best, won->face);
        won->best = better ? d : won->best;
        won->face = better ? f : won->face;
    }
};
NPCD_HD MdQuery md_query(const float* p, bool own) { return MdQuery{{p[0], p[1], p[2]}, md_point_slack(p), own}; }

}  // namespace npcd
