// The tiles of a triangle mesh that the query kernels walk: what the boxes launch of csrc/mesh_distance.hip leaves in
// the workspace, and what mesh_distance.hip and raycast.hip read from it.  Per-lane code for the device and the host: nothing of HIP.
//   Corners   a face takes part if its three indices lie in [0, V); the corners launch writes its nine coordinates as three 16-byte
//             words.  Every other face, and the padding of the last tile, is written as NaN: no pair with it ever wins.
//   Box       per tile of kMdTile consecutive faces the axis-aligned box of the corners that are finite, of the faces that take part,
//             and slack = 2^-20 the largest power of two at or below the largest |coordinate| among them: 8 ulp.
//   Layout    md_ws_layout: the boxes of all tiles, then the corners of all tiles, from a 16-byte aligned base.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bits.h"

namespace npcd {

constexpr int kMdTile = 256;                                  // faces per tile; the corners launch runs one workgroup of kMdTile lanes per tile
constexpr int64_t kMdMaxVertices = (int64_t)1 << 31;
constexpr int64_t kMdMaxFaces = (int64_t)1 << 28;
constexpr uint32_t kMdInfBits = 0x7f800000u;

struct alignas(16) MdCorner {          // one corner of a face: a 16-byte word, the fourth float is not read
    float x, y, z, pad;
};
struct alignas(16) MdBox {          // one tile
    float lo[3], slack, hi[3];
    int32_t count;          // the corners inside: 0 for a tile that is always skipped
};

NPCD_HD int64_t md_tiles(int64_t F) { return (F + kMdTile - 1) / kMdTile; }

struct TileWinner {          // what a lane of a nearest-face or first-hit query keeps while its wave walks the tiles (tile_walk.h)
    float best;          // +inf: no face won
    int32_t face;        // -1 then
};

struct MdWs {          // the workspace: 16-byte aligned base
    MdBox* boxes;              // [tiles]
    MdCorner* corners;         // [tiles * kMdTile, 3]
};
// -> the bytes of the workspace of F faces
static inline int64_t md_ws_layout(void* ws, int64_t F, MdWs* out) {
    const int64_t tiles = md_tiles(F);
    out->boxes = static_cast<MdBox*>(ws);
    out->corners = reinterpret_cast<MdCorner*>(out->boxes + tiles);
    return tiles * (int64_t)sizeof(MdBox) + tiles * kMdTile * 3 * (int64_t)sizeof(MdCorner);
}

// ---- one face of the corners launch -----------------------------------------------------------------------------------------------------
// out [3]: the corners of face f, NaN where the face does not take part (or f >= F).  -> true if it takes part
NPCD_HD bool md_corners_lane(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int64_t f, MdCorner* out) {
    const float nan = bits_float(0x7fc00000u);
    bool valid = f < F;
    int64_t idx[3] = {0, 0, 0};
    if (valid)
        for (int k = 0; k < 3; ++k) {
            idx[k] = faces[f * 3 + k];
            valid = valid && idx[k] >= 0 && idx[k] < V;
        }
    for (int k = 0; k < 3; ++k) {
        out[k].pad = 0.f;
        if (valid) {
            out[k].x = vertices[idx[k] * 3], out[k].y = vertices[idx[k] * 3 + 1], out[k].z = vertices[idx[k] * 3 + 2];
        } else {
            out[k].x = out[k].y = out[k].z = nan;
        }
    }
    return valid;
}
// a corner joins a box if its three coordinates are finite
NPCD_HD bool md_corner_counts(const MdCorner& c) { return is_finite(c.x) && is_finite(c.y) && is_finite(c.z); }
NPCD_HD uint32_t md_abs_bits(const MdCorner& c) {
    const uint32_t x = float_bits(c.x) & 0x7fffffffu, y = float_bits(c.y) & 0x7fffffffu, z = float_bits(c.z) & 0x7fffffffu;
    return x > y ? (x > z ? x : z) : (y > z ? y : z);
}
// 8 ulp of a finite |coordinate| given by its bits: 2^-20 of the power of two at or below it, at least 8 times the smallest float
NPCD_HD float md_slack(uint32_t abs_bits) {
    const float unit = bits_float(abs_bits & kMdInfBits) * 9.5367431640625e-07f;          // 2^-20, exact or a denormal power of two
    const float least = bits_float(8u);
    return unit > least ? unit : least;
}
NPCD_HD float md_point_slack(const float* p) {
    const MdCorner c = {p[0], p[1], p[2], 0.f};
    return md_corner_counts(c) ? md_slack(md_abs_bits(c)) : bits_float(8u);
}
// the box of `n` corners (n a multiple of three, NaN corners do not count)
NPCD_HD MdBox md_box_of(const MdCorner* corners, int64_t n) {
    const float inf = bits_float(kMdInfBits);
    MdBox box = {{inf, inf, inf}, 0.f, {-inf, -inf, -inf}, 0};
    uint32_t top = 0;
    for (int64_t j = 0; j < n; ++j) {
        const MdCorner& c = corners[j];
        if (!md_corner_counts(c)) continue;
        const float x[3] = {c.x, c.y, c.z};
        for (int k = 0; k < 3; ++k) box.lo[k] = x[k] < box.lo[k] ? x[k] : box.lo[k], box.hi[k] = x[k] > box.hi[k] ? x[k] : box.hi[k];
        const uint32_t m = md_abs_bits(c);
        top = m > top ? m : top;
        box.count += 1;
    }
    box.slack = md_slack(top);
    return box;
}

}  // namespace npcd
