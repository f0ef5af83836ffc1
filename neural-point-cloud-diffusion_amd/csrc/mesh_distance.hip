// The closest point of a triangle mesh to every query point.  The per-lane arithmetic is csrc/mesh_distance.h, shared
// with the host program csrc/mesh_distance_host.cpp; this file is the launches around it.  Compiled without FMA contraction and
// without packed fp32 (build.py).
//
//   npcd_mesh_distance_boxes, one launch: one workgroup of kMdTile lanes per tile of kMdTile consecutive faces.  A lane gathers its
//     face's corners (md_corners_lane) and writes them as three 16-byte words to the workspace, NaN for a face that does not take part
//     and for the padding of the last tile; the box of the tile's finite corners is an exact minimum and maximum over the wave
//     (wave_reduce64 of csrc/wave.h), then over the four waves through LDS.
//   npcd_mesh_distance_query<cull>, one launch: one workgroup is one wave, a lane owns one query point with its running (best, face).
//     The wave walks the tiles in ascending order.  With cull, every lane takes md_bound to the tile's box -- the boxes are read
//     through wave-uniform addresses, kMdScan at a time so that their loads are in flight together -- and the wave skips the tile
//     unless some lane md_needs it.  Before the walk every lane finds the tile with its smallest bound, and the wave evaluates those
//     tiles, each once: a lane would need its own anyway, and the walk then starts with a best near the final one (without this, a
//     wave whose points lie in two places evaluated everything between them: docs/experiments.md R35.1).  A tile that is evaluated
//     is copied to LDS, 12 KiB, a straight copy of its 16-byte words, and read back three words per face, every lane the same
//     address: a broadcast.  The winner is the lexicographic minimum of (dist2, face), so neither the order of the visits nor the
//     skipped tiles change it (DESIGN.md 5.18 holds the argument); its closest point is evaluated once more after the walk.
//   No float atomics, no scratch, no workgroup that waits on another.  `evaluated`, where given, takes one integer add per wave.
//
// Bounds.  The workspace holds md_tiles(F) boxes and md_tiles(F) * kMdTile faces of corners, every one written by the boxes launch: a
// tile copy reads whole tiles.  A face index is followed only after it is held to [0, V) (md_corners_lane); a lane past the last point
// reads no point, asks for no tile and writes nothing; a winner is a loop index below F.
#include "common.h"
#include "mesh_distance.h"

namespace npcd {

struct MdWs {          // the workspace: 16-byte aligned base
    MdBox* boxes;              // [tiles]
    MdCorner* corners;         // [tiles * kMdTile, 3]
};
static inline int64_t md_ws_layout(void* ws, int64_t F, MdWs* out) {
    const int64_t tiles = md_tiles(F);
    out->boxes = static_cast<MdBox*>(ws);
    out->corners = reinterpret_cast<MdCorner*>(out->boxes + tiles);
    return tiles * (int64_t)sizeof(MdBox) + tiles * kMdTile * 3 * (int64_t)sizeof(MdCorner);
}

__global__ __launch_bounds__(kMdTile) void md_boxes_kernel(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ faces,
                                                           int64_t F, MdWs ws) {
    __shared__ float part[kMdTile / 64][8];
    const int64_t f = (int64_t)blockIdx.x * kMdTile + threadIdx.x;
    MdCorner c[3];
    md_corners_lane(vertices, V, faces, F, f, c);
    for (int k = 0; k < 3; ++k) ws.corners[f * 3 + k] = c[k];          // f < tiles * kMdTile
    const MdBox own = md_box_of(c, 3);
    float v[8] = {own.lo[0], own.lo[1], own.lo[2], own.hi[0], own.hi[1], own.hi[2], 0.f, (float)own.count};
    for (int k = 0; k < 3; ++k)
        if (md_corner_counts(c[k])) v[6] = fmaxf(v[6], bits_float(md_abs_bits(c[k])));
    for (int k = 0; k < 3; ++k) v[k] = wave_reduce64(v[k], [](float a, float b) { return fminf(a, b); });
    for (int k = 3; k < 7; ++k) v[k] = wave_max64(v[k]);
    v[7] = wave_sum64(v[7]);          // at most 768: exact
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 8; ++k) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMdTile / 64; ++w) {
            for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], part[w][k]);
            for (int k = 3; k < 7; ++k) v[k] = fmaxf(v[k], part[w][k]);
            v[7] += part[w][7];
        }
        MdBox box = {{v[0], v[1], v[2]}, md_slack(float_bits(v[6])), {v[3], v[4], v[5]}, (int32_t)v[7]};
        ws.boxes[blockIdx.x] = box;
    }
}

struct MdArgs {
    const float* points;
    const MdBox* boxes;
    const MdCorner* corners;
    float *sqdist, *closest;
    int32_t* face;
    unsigned long long* evaluated;
    int64_t S, F;
};

// the wave copies tile t to LDS and every lane takes its faces; count = the faces of the tile below F
__device__ __forceinline__ void md_eval_tile(const MdArgs& a, int t, MdCorner* tile, const float* p, float& best, int32_t& best_face) {
    const f32x4* __restrict__ from = reinterpret_cast<const f32x4*>(a.corners + (int64_t)t * kMdTile * 3);
    f32x4* to = reinterpret_cast<f32x4*>(tile);
    __syncthreads();          // the tile before has been read
#pragma unroll
    for (int k = 0; k < kMdTile * 3 / kMdThreads; ++k) to[k * kMdThreads + threadIdx.x] = from[k * kMdThreads + threadIdx.x];
    __syncthreads();
    const int64_t left = a.F - (int64_t)t * kMdTile;
    const int count = left < kMdTile ? (int)left : kMdTile;
    const int base = t * kMdTile;
#pragma unroll 2
    for (int j = 0; j < count; ++j) {
        const MdCorner ca = tile[3 * j], cb = tile[3 * j + 1], cc = tile[3 * j + 2];
        const float fa[3] = {ca.x, ca.y, ca.z}, fb[3] = {cb.x, cb.y, cb.z}, fc[3] = {cc.x, cc.y, cc.z};
        float q[3];
        const float d = md_pair(p, fa, fb, fc, q);
        const bool better = md_better(d, base + j, best, best_face);
        best = better ? d : best;
        best_face = better ? base + j : best_face;
    }
}

template <bool CULL>
__global__ __launch_bounds__(kMdThreads) void md_query_kernel(MdArgs a) {
    __shared__ MdCorner tile[kMdTile * 3];
    const int64_t i = (int64_t)blockIdx.x * kMdThreads + threadIdx.x;
    const bool own = i < a.S;
    const float nan = bits_float(0x7fc00000u);
    const float p[3] = {own ? a.points[i * 3] : nan, own ? a.points[i * 3 + 1] : nan, own ? a.points[i * 3 + 2] : nan};
    const int tiles = (int)md_tiles(a.F);
    float best = bits_float(kMdInfBits);
    int32_t best_face = -1;
    unsigned evaluated = 0;
    const float point_slack = md_point_slack(p);
    int nearest = -1;
    if (CULL) {
        // every lane's tile with the smallest bound, the lowest such, is evaluated first: the lane would need it anyway, and the walk
        // then starts with a best that is near the final one
        float least = bits_float(kMdInfBits);
        for (int t0 = 0; t0 < tiles; t0 += kMdScan) {
            float bound[kMdScan];
#pragma unroll
            for (int k = 0; k < kMdScan; ++k) bound[k] = md_bound(p, point_slack, a.boxes[min(t0 + k, tiles - 1)]);
#pragma unroll
            for (int k = 0; k < kMdScan; ++k) {
                const bool nearer = own & (t0 + k < tiles) & (bound[k] < least);
                least = nearer ? bound[k] : least;
                nearest = nearer ? t0 + k : nearest;
            }
        }
        unsigned long long pending = __ballot(nearest >= 0);
        while (pending != 0) {          // wave-uniform: at most one trip per lane
            const int t = __builtin_amdgcn_readlane(nearest, __ffsll(pending) - 1);
            md_eval_tile(a, t, tile, p, best, best_face);
            evaluated += 1;
            pending &= ~__ballot(nearest == t);
        }
    }
    for (int t0 = 0; t0 < tiles; t0 += kMdScan) {
        float bound[kMdScan];
        if (CULL) {
#pragma unroll
            for (int k = 0; k < kMdScan; ++k) bound[k] = md_bound(p, point_slack, a.boxes[min(t0 + k, tiles - 1)]);
        }
#pragma unroll
        for (int k = 0; k < kMdScan; ++k) {
            const int t = t0 + k;
            if (t >= tiles) break;
            if (CULL) {
                if (__ballot(own & md_needs(bound[k], best)) == 0) continue;
                if (__ballot(nearest == t) != 0) continue;          // evaluated before the walk
            }
            md_eval_tile(a, t, tile, p, best, best_face);
            evaluated += 1;
        }
    }
    if (a.evaluated && threadIdx.x == 0 && evaluated) atomicAdd(a.evaluated, (unsigned long long)evaluated);
    if (!own) return;
    float q[3] = {0.f, 0.f, 0.f};
    if (best_face >= 0) {          // below F: a loop index
        const MdCorner* c = a.corners + (int64_t)best_face * 3;
        const float fa[3] = {c[0].x, c[0].y, c[0].z}, fb[3] = {c[1].x, c[1].y, c[1].z}, fc[3] = {c[2].x, c[2].y, c[2].z};
        md_pair(p, fa, fb, fc, q);
    }
    a.sqdist[i] = best;
    a.face[i] = best_face;
    a.closest[i * 3] = q[0], a.closest[i * 3 + 1] = q[1], a.closest[i * 3 + 2] = q[2];
}

static int md_check(int64_t V, int64_t F) {
    if (V < 0 || F < 0) return NPCD_ERR_ARG;
    // an index is an int32, a tile index an int
    if (V >= kMdMaxVertices || F >= kMdMaxFaces) return NPCD_ERR_UNSUPPORTED;
    return NPCD_OK;
}

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_mesh_distance_ws_bytes(int64_t V, int64_t F) {
    const int rc = md_check(V, F);
    if (rc != NPCD_OK) return rc;
    MdWs w;
    return md_ws_layout(nullptr, F, &w);
}

extern "C" int npcd_mesh_distance_boxes(const float* vertices, int64_t V, const int32_t* faces, int64_t F, void* ws, void* stream) {
    const int rc = md_check(V, F);
    if (rc != NPCD_OK) return rc;
    if (F < 1 || !faces || !ws || (V > 0 && !vertices)) return NPCD_ERR_ARG;
    if (misaligned(vertices, 4) || misaligned(faces, 4) || misaligned(ws, 16)) return NPCD_ERR_ARG;
    MdWs w;
    md_ws_layout(ws, F, &w);
    hipLaunchKernelGGL(md_boxes_kernel, dim3((unsigned)md_tiles(F)), dim3(kMdTile), 0, static_cast<hipStream_t>(stream), vertices, V, faces,
                       F, w);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_mesh_distance_query(const float* points, int64_t S, const float* vertices, int64_t V, const int32_t* faces, int64_t F,
                                        const void* ws, int cull, float* sqdist, int32_t* face, float* closest, int64_t* evaluated,
                                        void* stream) {
    const int rc = md_check(V, F);
    if (rc != NPCD_OK) return rc;
    if (S < 0) return NPCD_ERR_ARG;
    if (S >= kMdMaxPoints) return NPCD_ERR_UNSUPPORTED;
    if (S < 1 || F < 1 || !points || !ws || !sqdist || !face || !closest || (cull != 0 && cull != 1)) return NPCD_ERR_ARG;
    if (misaligned(points, 4) || misaligned(sqdist, 4) || misaligned(face, 4) || misaligned(closest, 4) ||
        misaligned(ws, 16) || misaligned(evaluated, 8))
        return NPCD_ERR_ARG;
    (void)vertices, (void)faces;          // the corners in the workspace are what the query reads
    MdWs w;
    md_ws_layout(const_cast<void*>(ws), F, &w);
    const MdArgs a{points, w.boxes, w.corners, sqdist, closest, face, reinterpret_cast<unsigned long long*>(evaluated), S, F};
    const dim3 grid(blocks_for(S, kMdThreads)), block(kMdThreads);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (cull)
        hipLaunchKernelGGL(md_query_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(md_query_kernel<false>, grid, block, 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
