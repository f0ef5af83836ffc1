// How often every ray crosses a triangle mesh, per facing: what tells inside from outside.  The per-lane arithmetic
// is csrc/raycast.h (rc_cross, CrQuery), shared with the host program csrc/crossings_host.cpp; this file is the launch around it.
// Compiled without FMA contraction and without packed fp32 (build.py).
//
//   npcd_crossings_query<cull>, one launch: one workgroup is one wave, a lane owns one ray (CrQuery) with two int32 counters and the
//     wave sweeps the tiles (tile_sweep of csrc/tile_walk.h, which holds the schedule, the LDS copy and the barriers): a tile is
//     evaluated iff the segment [t_min, t_max] of some lane's ray reaches its box.  The corners and the boxes are those that
//     npcd_mesh_distance_boxes (mesh_distance.hip) left in the workspace.  The outputs are counts of pairs that each pass a test of
//     their own, so neither the order of the visits nor the skipped tiles change them.
//   No float atomics, no scratch, no workgroup that waits on another.
//
// Bounds.  A lane past the last ray reads no ray, reaches no tile and writes nothing.  tile_walk.h holds those of the workspace.
#include "common.h"
#include "raycast.h"
#include "tile_walk.h"

namespace npcd {

struct CrArgs {
    const float *origins, *directions;
    const MdBox* boxes;
    const MdCorner* corners;
    int32_t *front, *back;
    unsigned long long* evaluated;
    int64_t R, F;
    float t_min, t_max;
};

template <bool CULL>
__global__ __launch_bounds__(kRcThreads) void cr_query_kernel(CrArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
    const bool own = i < a.R;
    const float nan = bits_float(0x7fc00000u);
    float o[3], d[3];
    for (int k = 0; k < 3; ++k) o[k] = own ? a.origins[i * 3 + k] : nan, d[k] = own ? a.directions[i * 3 + k] : nan;
    const CrQuery query{rc_ray(o, d), a.t_min, a.t_max};          // a lane past the last ray: not valid, reaches nothing
    const RcCrossings count = tile_sweep<CrQuery, CULL>(query, a.boxes, a.corners, a.F, a.evaluated);
    if (!own) return;
    a.front[i] = count.front;
    a.back[i] = count.back;
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_crossings_query(const float* origins, const float* directions, int64_t R, const float* vertices, int64_t V,
                                    const int32_t* faces, int64_t F, const void* ws, float t_min, float t_max, int cull, int32_t* front,
                                    int32_t* back, int64_t* evaluated, void* stream) {
    if (V < 0 || F < 0 || R < 0) return NPCD_ERR_ARG;
    if (V >= kMdMaxVertices || F >= kMdMaxFaces || R >= kRcMaxRays) return NPCD_ERR_UNSUPPORTED;
    if (R < 1 || F < 1 || !origins || !directions || !ws || !front || !back || (cull != 0 && cull != 1)) return NPCD_ERR_ARG;
    if (misaligned(origins, 4) || misaligned(directions, 4) || misaligned(front, 4) || misaligned(back, 4) || misaligned(ws, 16) ||
        misaligned(evaluated, 8))
        return NPCD_ERR_ARG;
    (void)vertices, (void)faces;          // the corners in the workspace are what the query reads
    MdWs w;
    md_ws_layout(const_cast<void*>(ws), F, &w);
    const CrArgs a{origins, directions, w.boxes, w.corners, front, back, reinterpret_cast<unsigned long long*>(evaluated), R, F, t_min, t_max};
    const dim3 grid(blocks_for(R, kRcThreads)), block(kRcThreads);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (cull)
        hipLaunchKernelGGL(cr_query_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(cr_query_kernel<false>, grid, block, 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
