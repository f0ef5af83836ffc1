// Area-weighted sampling of triangle meshes: the per-lane arithmetic of csrc/surface.hip, written once for the device
// and the host.  The kernels run these functions one lane per face, tile entry or sample; the stand-alone program
// csrc/surface_host.cpp runs them as plain loops over tiles and lanes (tests/test_surface_sampling_cpu.py): this header includes
// nothing of HIP.  All fp32 arithmetic is as written -- the file is compiled without FMA contraction (build.py) -- sqrt and the
// divisions are the correctly rounded ones.
//
//   Face measure   e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2, d = sqrt((nx nx + ny ny) + nz nz) = twice the area; +0 where that is
//                  not finite or an index lies outside [0, V) -- no vertex is read through such an index.
//   Weights        d_max = the largest d of the mesh (an integer maximum on the bits: d >= +0), k = 31 - floor(log2 d_max) from the
//                  exponent of float64(d_max), w = floor(float64(d) 2^k) < 2^32: integers, so every order of summation gives the
//                  same prefix sums.  Per tile of kSurfTile faces the inclusive sums of w (local to the tile, < 2^40), per mesh the
//                  inclusive sums of the tile totals, W the last of them (< 2^63).
//   Sample         k0 = clamp(floor(u0 2^24), 0, 2^24 - 1) (NaN: 0), r = floor(k0 W / 2^24) < W, the face the smallest i whose
//                  inclusive sum exceeds r: the tile by an upper-bound search over the tile sums, the face by one over the tile's
//                  local sums with r less the sum before the tile.  s = sqrt(u1), b = (1 - s, s (1 - u2), s u2), and every output
//                  row is (b0 x0 + b1 x1) + b2 x2 of the three corners' rows.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bits.h"

namespace npcd {

// faces per tile = lanes per workgroup of the quantise launch: one wave scan per wave and one LDS step over the four wave totals.  The
// sample's second search then walks 8 entries of one 2-KB run of local sums.
constexpr int kSurfTile = 256;
constexpr int kSurfThreads = 256;
// tile sums a sampling workgroup stages in LDS (32 KB): meshes of up to kSurfLdsTiles * kSurfTile = 1,048,576 faces are searched
// there, larger ones in global memory
constexpr int kSurfLdsTiles = 4096;
constexpr int kSurfMaxChannels = 16;
enum { kSurfNormalsNone = 0, kSurfNormalsFace = 1, kSurfNormalsVertex = 2 };

// the first tile slot of mesh b: the meshes before it fill at most floor(face_offset / kSurfTile) + b slots, and the slots of
// consecutive meshes do not overlap; floor(F_total / kSurfTile) + B slots hold a batch
NPCD_HD int64_t surf_tile_base(int face_offset, int b) { return (int64_t)(face_offset / kSurfTile) + b; }
NPCD_HD int surf_tiles(int faces) { return faces / kSurfTile + (faces % kSurfTile != 0); }
NPCD_HD int64_t surf_slots(int B, int F_total) { return (int64_t)(F_total / kSurfTile) + B; }

// rows [first, first + count) of member b in a packed array of `total` rows; offsets [B + 1] that do not ascend inside
// [0, total] give an empty member: nothing is read or written through them
struct SurfSpan {
    int first, count;
};
NPCD_HD SurfSpan surf_span(const int32_t* offsets, int b, int total) {
    const int lo = offsets[b], hi = offsets[b + 1];
    SurfSpan s;
    s.first = 0, s.count = 0;
    if (lo >= 0 && hi >= lo && hi <= total) s.first = lo, s.count = hi - lo;
    return s;
}
// the member that owns tile slot `slot`: the largest b whose first slot is not above it (the bases ascend strictly with b); the slot
// is one of its tiles iff slot - base < surf_tiles(F_b)
NPCD_HD int surf_slot_member(const int32_t* face_offsets, int B, int64_t slot) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (surf_tile_base(face_offsets[mid], mid) <= slot) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct SurfFace {
    float v[3][3];          // the three corners
    float n[3], d;          // e1 x e2 and its length
};
// the corners, normal and measure of a face; false (and d = +0, nothing read) if an index lies outside [0, V)
NPCD_HD bool surf_face(const float* vertices, const int32_t* face, int V, SurfFace* f) {
    const int i0 = face[0], i1 = face[1], i2 = face[2];
    f->d = 0.f;
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    for (int a = 0; a < 3; ++a) f->v[0][a] = vertices[(int64_t)i0 * 3 + a], f->v[1][a] = vertices[(int64_t)i1 * 3 + a], f->v[2][a] = vertices[(int64_t)i2 * 3 + a];
    const float e1x = f->v[1][0] - f->v[0][0], e1y = f->v[1][1] - f->v[0][1], e1z = f->v[1][2] - f->v[0][2];
    const float e2x = f->v[2][0] - f->v[0][0], e2y = f->v[2][1] - f->v[0][1], e2z = f->v[2][2] - f->v[0][2];
    f->n[0] = e1y * e2z - e1z * e2y, f->n[1] = e1z * e2x - e1x * e2z, f->n[2] = e1x * e2y - e1y * e2x;
    const float d = sqrtf((f->n[0] * f->n[0] + f->n[1] * f->n[1]) + f->n[2] * f->n[2]);
    f->d = d < INFINITY ? d : 0.f;          // NaN and +inf: no measure
    return true;
}
NPCD_HD float surf_face_measure(const float* vertices, const int32_t* face, int V) {
    SurfFace f;
    surf_face(vertices, face, V, &f);
    return f.d;
}

// k = 31 - floor(log2 d_max) for d_max > 0: d_max maps into [2^31, 2^32); -96 .. 180
NPCD_HD int surf_shift(float d_max) { return 31 - floor_log2(d_max); }
// w = floor(float64(d) 2^k): the product is exact, d_max maps into [2^31, 2^32); a mesh without measure (d_max = 0) has w = 0
NPCD_HD uint64_t surf_quantise(float d, uint32_t d_max_bits) {
    if (d_max_bits == 0) return 0;
    return (uint64_t)((double)d * pow2(surf_shift(bits_float(d_max_bits))));
}
// area = 0.5 float64(W) 2^-k
NPCD_HD double surf_area(uint64_t W, uint32_t d_max_bits) {
    if (d_max_bits == 0) return 0.0;
    return 0.5 * (double)W * pow2(-surf_shift(bits_float(d_max_bits)));
}

NPCD_HD uint32_t surf_k0(float u0) {
    const float t = floorf(u0 * 16777216.f);
    return !(t > 0.f) ? 0u : t >= 16777215.f ? 16777215u : (uint32_t)t;
}
// floor(k0 W / 2^24) for k0 < 2^24 and W < 2^63, exactly.  The product has up to 87 bits; with W = Whi 2^32 + Wlo it is
// (k0 Whi) 2^32 + k0 Wlo, both products below 2^56, and the first term is a multiple of 2^24: floor((k0 Whi) 2^8 + k0 Wlo / 2^24)
// = (k0 Whi) 2^8 + floor(k0 Wlo / 2^24) -- the high and the low half of the 128-bit product, without the 128-bit multiply
NPCD_HD uint64_t surf_mul_shift(uint32_t k0, uint64_t W) {
    const uint64_t hi = (uint64_t)k0 * (W >> 32), lo = (uint64_t)k0 * (W & 0xffffffffu);
    return (hi << 8) + (lo >> 24);
}
// the smallest i in [0, n) with a[i] > r, n if there is none; a ascending
NPCD_HD int surf_upper_bound(const uint64_t* a, int n, uint64_t r) {
    int lo = 0, hi = n;
    while (lo < hi) {          // a[i] <= r for i < lo, a[i] > r for i >= hi
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

NPCD_HD void surf_barycentric(float u1, float u2, float* b) {
    const float s = sqrtf(u1);
    b[0] = 1.f - s, b[1] = s * (1.f - u2), b[2] = s * u2;
}
NPCD_HD float surf_mix(const float* b, float x0, float x1, float x2) { return (b[0] * x0 + b[1] * x1) + b[2] * x2; }

// ---- one face of the measure launch -------------------------------------------------------------------------------------------------
// -> the bits of d, for the mesh's integer maximum; d goes to d_out
NPCD_HD uint32_t surf_measure_lane(const float* vertices, const int32_t* faces, int V, int face, float* d_out) {
    const float d = surf_face_measure(vertices, faces + (int64_t)face * 3, V);
    d_out[face] = d;
    return float_bits(d);
}

// ---- one sample --------------------------------------------------------------------------------------------------------------------
struct SurfMesh {          // one member of the batch, pointers at its own first row
    const float* vertices;          // [V, 3]
    const int32_t* faces;           // [F, 3]
    const uint64_t* local;          // [F] inclusive sums of w inside every tile
    const uint64_t* tiles;          // [surf_tiles(F)] inclusive sums of the tile totals; may point at a staged copy
    const float* vnormals;          // [V, 3] or null
    const float* attrs;             // [V, C] or null
    int V, F, C, normals_mode;
    uint64_t W;
};
struct SurfRow {          // where a sample's outputs go; null where an output is not asked for
    float* point;          // [3]
    int32_t* face;
    float* normal;         // [3]
    float* attr;           // [C]
};
NPCD_HD void surf_row_empty(const SurfMesh& m, const SurfRow& o) {
    o.point[0] = o.point[1] = o.point[2] = 0.f;
    if (o.face) *o.face = -1;
    if (o.normal) o.normal[0] = o.normal[1] = o.normal[2] = 0.f;
    if (o.attr) for (int c = 0; c < m.C; ++c) o.attr[c] = 0.f;
}
NPCD_HD void surf_sample_row(const SurfMesh& m, const float* u, const SurfRow& o) {
    if (m.W == 0) return surf_row_empty(m, o);
    const uint64_t r = surf_mul_shift(surf_k0(u[0]), m.W);          // r < W: a tile's sum exceeds it
    int tile = surf_upper_bound(m.tiles, surf_tiles(m.F), r);
    if (tile >= surf_tiles(m.F)) tile = surf_tiles(m.F) - 1;          // (cannot be: sums that are not those of this mesh)
    const uint64_t before = tile ? m.tiles[tile - 1] : 0;
    const int first = tile * kSurfTile, count = m.F - first < kSurfTile ? m.F - first : kSurfTile;
    int face = first + surf_upper_bound(m.local + first, count, r - before);
    if (face >= m.F) face = m.F - 1;
    SurfFace f;
    if (!surf_face(m.vertices, m.faces + (int64_t)face * 3, m.V, &f)) return surf_row_empty(m, o);          // (cannot be: its w is 0)
    float b[3];
    surf_barycentric(u[1], u[2], b);
    for (int a = 0; a < 3; ++a) o.point[a] = surf_mix(b, f.v[0][a], f.v[1][a], f.v[2][a]);
    if (o.face) *o.face = face;
    const int32_t* idx = m.faces + (int64_t)face * 3;
    if (o.normal && m.normals_mode == kSurfNormalsFace) {
        for (int a = 0; a < 3; ++a) o.normal[a] = f.n[a] / f.d;          // (a chosen face has w > 0: d is finite)
    } else if (o.normal) {
        const float *g0 = m.vnormals + (int64_t)idx[0] * 3, *g1 = m.vnormals + (int64_t)idx[1] * 3, *g2 = m.vnormals + (int64_t)idx[2] * 3;
        const float gx = surf_mix(b, g0[0], g1[0], g2[0]), gy = surf_mix(b, g0[1], g1[1], g2[1]), gz = surf_mix(b, g0[2], g1[2], g2[2]);
        const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
        float nx = gx / len, ny = gy / len, nz = gz / len;
        if (!(fabsf(nx) < INFINITY && fabsf(ny) < INFINITY && fabsf(nz) < INFINITY)) nx = ny = nz = 0.f;
        o.normal[0] = nx, o.normal[1] = ny, o.normal[2] = nz;
    }
    if (o.attr) {
        const float *a0 = m.attrs + (int64_t)idx[0] * m.C, *a1 = m.attrs + (int64_t)idx[1] * m.C, *a2 = m.attrs + (int64_t)idx[2] * m.C;
        for (int c = 0; c < m.C; ++c) o.attr[c] = surf_mix(b, a0[c], a1[c], a2[c]);
    }
}

}  // namespace npcd
