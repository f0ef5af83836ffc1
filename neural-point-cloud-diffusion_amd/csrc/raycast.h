// The first intersection of a ray with a triangle mesh: the per-lane arithmetic of csrc/raycast.hip, written once for
// the device and the host.  The kernel runs these functions one lane per ray; the stand-alone program csrc/raycast_host.cpp runs them
// as plain loops (tests/test_raycast_cpu.py): this header includes nothing of HIP.  All arithmetic is as written -- the file is
// compiled without FMA contraction (build.py) -- and the divisions are the correctly rounded ones.
//
//   Ray       rc_ray: kz the axis of the largest |d|, the lowest among equal ones, kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped if
//             d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz] in fp32.  A ray with a component of o or d that is not
//             finite, or with d[kz] == 0, hits nothing.
//   Pair      rc_pair: per corner p = P - o, px = p[kx] - Sx p[kz], py = p[ky] - Sy p[kz], pz = Sz p[kz] in fp32; the edge functions
//             U = cx by - cy bx, V = ax cy - ay cx, W = bx ay - by ax in fp64 (the products are exact, so the signs are), det =
//             (U + V) + W.  Outside if one of U, V, W is below 0 and another above, if det == 0 or anything is NaN.  Inside:
//             T = (U az + V bz) + W cz and t = float(T / det).  A hit iff t_min <= t <= t_max and t < +inf (rc_hit).
//   Winner    the lexicographic minimum of (t, face) over the hits, t ordered as a signed float with -0 == +0: rc_better on two
//             words, rc_key on one.  t_min may be negative.
//   Reach     rc_reach: the slab test of the segment [from, to] of a ray against a tile's box (mesh_tiles.h) enlarged by
//             kRcSlack times the larger of the box's and the origin's 8 ulp, at least kRcSlackFloor; DESIGN.md 5.19 derives why no
//             hit of the pair rule lies outside it.  A ray that is not tame (|d[kz]| outside [2^-40, 2^40]) reaches every box.
//   Query     RcQuery: a lane's ray and limits, and the answers of these functions to the tile walk (tile_walk.h).
//   Crossing  rc_cross: the counting form of the pair on the same corners, U, V, W, det and t: a half-open rule in
//             place of the inclusive one, so that every crossing of a closed surface is counted once.  CrQuery (csrc/crossings.hip)
//             counts those with rc_hit per facing; every crossing is a hit of rc_pair, so rc_reach culls none.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bits.h"
#include "mesh_tiles.h"

namespace npcd {

constexpr int kRcThreads = 64;          // lanes per workgroup: one wave, one ray per lane
constexpr int kRcScan = 4;              // boxes a wave tests at a time: their loads are in flight together
constexpr int64_t kRcMaxRays = (int64_t)1 << 31;
constexpr float kRcSlack = 4.0f;                 // times 8 ulp of the largest |coordinate|: 32 ulp
constexpr uint32_t kRcSlackFloorBits = 0x0d800000u;          // 2^-100
constexpr uint32_t kRcTameLoBits = 0x2b800000u, kRcTameHiBits = 0x53800000u;          // 2^-40 and 2^40
constexpr uint64_t kRcNoKey = ~(uint64_t)0;          // what a ray without a hit keeps: above every key of a hit

struct RcRay {
    float o[3], d[3];
    int kx, ky, kz;
    float Sx, Sy, Sz;
    bool valid;          // it can hit
    bool tame;           // rc_reach may cull for it
    float inv[3];        // 1 / d per axis
    float slack;         // 8 ulp of the origin's largest |coordinate|
};

struct RcPair {
    double U, V, W, det;
    float t;             // NaN outside
    bool inside;
};

NPCD_HD float rc_sel(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }

NPCD_HD RcRay rc_ray(const float* o, const float* d) {
    RcRay r;
    for (int k = 0; k < 3; ++k) r.o[k] = o[k], r.d[k] = d[k];
    const float a0 = fabsf(d[0]), a1 = fabsf(d[1]), a2 = fabsf(d[2]);
    int kz = 0;
    float top = a0;
    kz = a1 > top ? 1 : kz, top = a1 > top ? a1 : top;
    kz = a2 > top ? 2 : kz, top = a2 > top ? a2 : top;
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    const float dz = rc_sel(kz, d[0], d[1], d[2]);
    if (dz < 0.f) {
        const int s = kx;
        kx = ky, ky = s;
    }
    r.kx = kx, r.ky = ky, r.kz = kz;
    r.Sx = rc_sel(kx, d[0], d[1], d[2]) / dz;
    r.Sy = rc_sel(ky, d[0], d[1], d[2]) / dz;
    r.Sz = 1.f / dz;
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && is_finite(o[k]) && is_finite(d[k]);
    r.valid = finite & (dz != 0.f);
    r.tame = r.valid && top >= bits_float(kRcTameLoBits) && top <= bits_float(kRcTameHiBits);
    for (int k = 0; k < 3; ++k) r.inv[k] = 1.f / d[k];
    r.slack = md_point_slack(o);
    return r;
}

// ---- one pair -------------------------------------------------------------------------------------------------------------------------
NPCD_HD void rc_project(const RcRay& r, const float* P, float* out) {
    const float p0 = P[0] - r.o[0], p1 = P[1] - r.o[1], p2 = P[2] - r.o[2];
    const float pz = rc_sel(r.kz, p0, p1, p2);
    out[0] = rc_sel(r.kx, p0, p1, p2) - r.Sx * pz;
    out[1] = rc_sel(r.ky, p0, p1, p2) - r.Sy * pz;
    out[2] = r.Sz * pz;
}

// the sheared corners a, b, c [3] and the edge functions of a pair -> whether the ray is valid, none of them is a NaN and det != 0
NPCD_HD bool rc_edges(const RcRay& r, const float* A, const float* B, const float* C, float* a, float* b, float* c, RcPair* p) {
    rc_project(r, A, a), rc_project(r, B, b), rc_project(r, C, c);
    const double ax = a[0], ay = a[1], bx = b[0], by = b[1], cx = c[0], cy = c[1];
    p->U = cx * by - cy * bx;
    p->V = ax * cy - ay * cx;
    p->W = bx * ay - by * ax;
    p->det = (p->U + p->V) + p->W;
    const bool numbers = (p->U == p->U) & (p->V == p->V) & (p->W == p->W);          // det is then a NaN only if it is inf - inf
    return r.valid & numbers & (p->det != 0.0) & (p->det == p->det);
}
// t of a pair that `inside` keeps, NaN for the others
NPCD_HD void rc_depth(RcPair* p, bool inside, const float* a, const float* b, const float* c) {
    p->inside = inside;
    p->t = bits_float(0x7fc00000u);
    if (inside) {          // few pairs come here, and the float64 division costs as much as the edge functions: a branch, not a select
        const double T = (p->U * (double)a[2] + p->V * (double)b[2]) + p->W * (double)c[2];
        p->t = (float)(T / p->det);
    }
}

NPCD_HD RcPair rc_pair(const RcRay& r, const float* A, const float* B, const float* C) {
    float a[3], b[3], c[3];
    RcPair p;
    const bool sound = rc_edges(r, A, B, C, a, b, c, &p);
    const bool below = (p.U < 0.0) | (p.V < 0.0) | (p.W < 0.0), above = (p.U > 0.0) | (p.V > 0.0) | (p.W > 0.0);
    rc_depth(&p, sound & !(below & above), a, b, c);
    return p;
}

// does the directed edge start -> end, whose edge function at the origin is E, own the origin?  `pos`: det > 0; otherwise E and the
// edge are turned.  On the edge itself (E == 0) the top-left rule decides, from comparisons of the sheared coordinates
NPCD_HD bool rc_owns(double E, bool pos, const float* start, const float* end) {
    const bool strict = pos ? E > 0.0 : E < 0.0;
    const bool up = pos ? end[1] > start[1] : end[1] < start[1];            // dy > 0
    const bool left = pos ? end[0] < start[0] : end[0] > start[0];          // dx < 0
    return strict | ((E == 0.0) & (up | ((end[1] == start[1]) & left)));
}
// the counting form of rc_pair: the same corners, edge functions, det and t; inside iff every edge owns the origin,
// so that of the faces around a shared edge or vertex exactly one is crossed, and a face of no projected area never is
NPCD_HD RcPair rc_cross(const RcRay& r, const float* A, const float* B, const float* C) {
    float a[3], b[3], c[3];
    RcPair p;
    const bool sound = rc_edges(r, A, B, C, a, b, c, &p);
    const bool pos = p.det > 0.0;
    const bool u = rc_owns(p.U, pos, c, b), v = rc_owns(p.V, pos, a, c), w = rc_owns(p.W, pos, b, a);          // c -> b, a -> c, b -> a
    rc_depth(&p, sound & u & v & w, a, b, c);
    return p;
}
NPCD_HD bool rc_hit(float t, float t_min, float t_max) { return (t >= t_min) & (t <= t_max) & (t < bits_float(kMdInfBits)); }
// the weights of A, B, C and the facing of an inside pair
NPCD_HD void rc_finish(const RcPair& p, float* bary, int8_t* front) {
    bary[0] = (float)(p.U / p.det), bary[1] = (float)(p.V / p.det), bary[2] = (float)(p.W / p.det);
    *front = p.det > 0.0 ? 1 : 0;
}

// ---- the winner -----------------------------------------------------------------------------------------------------------------------
// a hit (t, face) replaces (best, best_face) if it is below it lexicographically
NPCD_HD bool rc_better(float t, int32_t face, float best, int32_t best_face) { return (t < best) | ((t == best) & (face < best_face)); }
// the same order on one word for a hit: the bits of t with the sign bit turned for t >= 0 and all bits for t < 0, either zero as +0
NPCD_HD uint64_t rc_key(float t, int32_t face) {
    uint32_t u = t == 0.f ? 0u : float_bits(t);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)face;
}

// ---- one (ray, tile) ------------------------------------------------------------------------------------------------------------------
// can a hit with from <= t <= to lie in the box?  *enter: where the ray enters the enlarged box, at least `from`
NPCD_HD bool rc_reach(const RcRay& r, const MdBox& box, float from, float to, float* enter) {
    const float inf = bits_float(kMdInfBits);
    *enter = from;
    if (!r.valid | (box.count == 0)) return false;
    if (!r.tame) return from <= to;
    const float larger = box.slack > r.slack ? box.slack : r.slack;
    const float wide = kRcSlack * larger, least = bits_float(kRcSlackFloorBits);
    const float slack = wide > least ? wide : least;
    float lo = from, hi = to;
    bool beside = false;
    for (int k = 0; k < 3; ++k) {
        const float n1 = (box.lo[k] - slack) - r.o[k], n2 = (box.hi[k] + slack) - r.o[k];
        const float a = n1 * r.inv[k], b = n2 * r.inv[k];
        const bool still = r.d[k] == 0.f, numbers = (a == a) & (b == b);
        beside = beside | (still & ((n1 > 0.f) | (n2 < 0.f)));          // a ray that does not move along k lies beside the slab
        const bool use = !still & numbers;
        const float near = use ? (a < b ? a : b) : -inf, far = use ? (a < b ? b : a) : inf;
        lo = near > lo ? near : lo;
        hi = far < hi ? far : hi;
    }
    *enter = lo;
    return !beside & (lo <= hi);
}

// ---- what the tile walk asks of a ray (tile_walk.h on the device, host_lanes.h on the host) --------------------------
struct RcQuery {
    static constexpr int kLanes = kRcThreads, kScan = kRcScan;
    typedef TileWinner State;
    typedef bool Memo;          // whether [t_min, min(best, t_max)] reaches a box, best of the scan group's start: one shrunk since asks for less
    RcRay ray;                  // of a lane without a ray: not valid, ranks no box and needs no tile
    float t_min, t_max;
    NPCD_HD bool rank(const MdBox& box, float* enter) const { return rc_reach(ray, box, t_min, t_max, enter); }
    NPCD_HD Memo recall(const MdBox& box, float best) const {
        float enter;
        return rc_reach(ray, box, t_min, best < t_max ? best : t_max, &enter);
    }
    NPCD_HD bool needs(Memo reach, float) const { return reach; }
    NPCD_HD RcPair pair(const MdCorner* c) const {          // with the face of corners c [3]
        const float fa[3] = {c[0].x, c[0].y, c[0].z}, fb[3] = {c[1].x, c[1].y, c[1].z}, fc[3] = {c[2].x, c[2].y, c[2].z};
        return rc_pair(ray, fa, fb, fc);
    }
    NPCD_HD void face(const MdCorner* c, int32_t f, State* won) const {
        const RcPair p = pair(c);
        const bool better = p.inside && rc_hit(p.t, t_min, t_max) && rc_better(p.t, f, won->best, won->face);
        won->best = better ? p.t : won->best;
        won->face = better ? f : won->face;
    }
};

// ---- counting crossings (crossings.hip): the need of a lane never shrinks, so the wave sweeps (tile_sweep) ---------------
struct RcCrossings {
    int32_t front, back;          // the counted crossings with det > 0 and with det < 0
};
struct CrQuery {
    static constexpr int kLanes = kRcThreads, kScan = kRcScan;
    typedef RcCrossings State;
    RcRay ray;                  // of a lane without a ray: not valid, reaches no box
    float t_min, t_max;
    NPCD_HD bool reaches(const MdBox& box) const {
        float enter;
        return rc_reach(ray, box, t_min, t_max, &enter);
    }
    NPCD_HD RcPair pair(const MdCorner* c) const {
        const float fa[3] = {c[0].x, c[0].y, c[0].z}, fb[3] = {c[1].x, c[1].y, c[1].z}, fc[3] = {c[2].x, c[2].y, c[2].z};
        return rc_cross(ray, fa, fb, fc);
    }
    NPCD_HD void face(const MdCorner* c, int32_t, State* count) const {
        const RcPair p = pair(c);
        const bool counted = p.inside && rc_hit(p.t, t_min, t_max), pos = p.det > 0.0;          // an inside pair has det != 0
        count->front += (counted & pos) ? 1 : 0;
        count->back += (counted & !pos) ? 1 : 0;
    }
};

}  // namespace npcd
