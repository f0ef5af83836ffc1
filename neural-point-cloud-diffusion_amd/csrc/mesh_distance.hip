// The closest point of a triangle mesh to every query point.  The per-lane arithmetic is csrc/mesh_tiles.h and
// csrc/mesh_distance.h, shared with the host program csrc/mesh_distance_host.cpp; this file is the launches around it.  Compiled
// without FMA contraction and without packed fp32 (build.py).
//
//   npcd_mesh_distance_boxes, one launch: one workgroup of kMdTile lanes per tile of kMdTile consecutive faces.  A lane gathers its
//     face's corners (md_corners_lane) and writes them as three 16-byte words to the workspace, NaN for a face that does not take part
//     and for the padding of the last tile; the box of the tile's finite corners is an exact minimum and maximum over the wave
//     (wave_reduce64 of csrc/wave.h), then over the four waves through LDS.
//   npcd_mesh_distance_query<cull>, one launch: one workgroup is one wave, a lane owns one query point (MdQuery) and the wave walks
//     the tiles (tile_walk of csrc/tile_walk.h, which holds the schedule, the LDS copy and the barriers).  The winner is the
//     lexicographic minimum of (dist2, face), so neither the order of the visits nor the skipped tiles change it (DESIGN.md 5.18
//     holds the argument); its closest point is evaluated once more after the walk.
//   No float atomics, no scratch, no workgroup that waits on another.
//
// Bounds.  A face index is followed only after it is held to [0, V) (md_corners_lane); a lane past the last point reads no point, asks
// for no tile and writes nothing; a winner is a loop index below F.  tile_walk.h holds those of the workspace.
#include "common.h"
#include "mesh_distance.h"
#include "tile_walk.h"

namespace npcd {

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

template <bool CULL>
__global__ __launch_bounds__(kMdThreads) void md_query_kernel(MdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kMdThreads + threadIdx.x;
    const bool own = i < a.S;
    const float nan = bits_float(0x7fc00000u);
    const float p[3] = {own ? a.points[i * 3] : nan, own ? a.points[i * 3 + 1] : nan, own ? a.points[i * 3 + 2] : nan};
    const MdQuery query = md_query(p, own);
    const TileWinner won = tile_walk<MdQuery, CULL>(query, a.boxes, a.corners, a.F, a.evaluated);
    if (!own) return;
    float q[3] = {0.f, 0.f, 0.f};
    if (won.face >= 0) query.pair(a.corners + (int64_t)won.face * 3, q);          // below F: a loop index
    a.sqdist[i] = won.best;
    a.face[i] = won.face;
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
