// The first intersection of every ray with a triangle mesh.  The per-lane arithmetic is csrc/raycast.h, shared with
// the host program csrc/raycast_host.cpp; this file is the launch around it.  Compiled without FMA contraction and without packed
// fp32 (build.py).
//
//   npcd_raycast_query<cull>, one launch: one workgroup is one wave, a lane owns one ray (RcQuery) and the wave walks the tiles
//     (tile_walk of csrc/tile_walk.h, which holds the schedule, the LDS copy and the barriers).  The corners and the boxes are those
//     that npcd_mesh_distance_boxes (mesh_distance.hip) left in the workspace.  The winner is the lexicographic minimum of (t, face)
//     over the hits, so neither the order of the visits nor the skipped tiles change it; its weights and facing are evaluated once
//     more after the walk.
//   No float atomics, no scratch, no workgroup that waits on another.
//
// Bounds.  A lane past the last ray reads no ray, reaches no tile and writes nothing; a winner is a loop index below F.  tile_walk.h
// holds those of the workspace.
#include "common.h"
#include "raycast.h"
#include "tile_walk.h"

namespace npcd {

struct RcArgs {
    const float *origins, *directions;
    const MdBox* boxes;
    const MdCorner* corners;
    float *t, *bary;
    int32_t* face;
    int8_t* front;
    unsigned long long* evaluated;
    int64_t R, F;
    float t_min, t_max;
};

template <bool CULL>
__global__ __launch_bounds__(kRcThreads) void rc_query_kernel(RcArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
    const bool own = i < a.R;
    const float nan = bits_float(0x7fc00000u);
    float o[3], d[3];
    for (int k = 0; k < 3; ++k) o[k] = own ? a.origins[i * 3 + k] : nan, d[k] = own ? a.directions[i * 3 + k] : nan;
    const RcQuery query{rc_ray(o, d), a.t_min, a.t_max};          // a lane past the last ray: not valid, reaches nothing
    const TileWinner won = tile_walk<RcQuery, CULL>(query, a.boxes, a.corners, a.F, a.evaluated);
    if (!own) return;
    float t = bits_float(kMdInfBits), bary[3] = {0.f, 0.f, 0.f};
    int8_t front = 0;
    if (won.face >= 0) {          // below F: a loop index
        const RcPair p = query.pair(a.corners + (int64_t)won.face * 3);
        t = p.t;
        rc_finish(p, bary, &front);
    }
    a.t[i] = t;
    a.face[i] = won.face;
    a.front[i] = front;
    a.bary[i * 3] = bary[0], a.bary[i * 3 + 1] = bary[1], a.bary[i * 3 + 2] = bary[2];
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_raycast_query(const float* origins, const float* directions, int64_t R, const float* vertices, int64_t V,
                                  const int32_t* faces, int64_t F, const void* ws, float t_min, float t_max, int cull, float* t, int32_t* face,
                                  float* bary, int8_t* front, int64_t* evaluated, void* stream) {
    if (V < 0 || F < 0 || R < 0) return NPCD_ERR_ARG;
    if (V >= kMdMaxVertices || F >= kMdMaxFaces || R >= kRcMaxRays) return NPCD_ERR_UNSUPPORTED;
    if (R < 1 || F < 1 || !origins || !directions || !ws || !t || !face || !bary || !front || (cull != 0 && cull != 1)) return NPCD_ERR_ARG;
    if (misaligned(origins, 4) || misaligned(directions, 4) || misaligned(t, 4) || misaligned(face, 4) || misaligned(bary, 4) ||
        misaligned(ws, 16) || misaligned(evaluated, 8))
        return NPCD_ERR_ARG;
    (void)vertices, (void)faces;          // the corners in the workspace are what the query reads
    MdWs w;
    md_ws_layout(const_cast<void*>(ws), F, &w);
    const RcArgs a{origins, directions, w.boxes, w.corners, t, bary, face, front, reinterpret_cast<unsigned long long*>(evaluated), R, F, t_min, t_max};
    const dim3 grid(blocks_for(R, kRcThreads)), block(kRcThreads);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (cull)
        hipLaunchKernelGGL(rc_query_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(rc_query_kernel<false>, grid, block, 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
