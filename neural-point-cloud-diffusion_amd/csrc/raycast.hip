// The first intersection of every ray with a triangle mesh.  The per-lane arithmetic is csrc/raycast.h, shared with
// the host program csrc/raycast_host.cpp; this file is the launch around it.  Compiled without FMA contraction and without packed
// fp32 (build.py).
//
//   npcd_raycast_query<cull>, one launch: one workgroup is one wave, a lane owns one ray with its running (best t, face).  The
//     corners and the boxes are those that npcd_mesh_distance_boxes (mesh_distance.hip) left in the workspace.  The wave walks the
//     tiles in ascending order.  With cull, every lane tests its segment [t_min, min(t_max, best)] against the tile's box (rc_reach)
//     -- the boxes are read through wave-uniform addresses, kRcScan at a time -- and the wave skips the tile unless some lane
//     reaches it.  Before the walk every lane finds the tile that its ray enters first, and the wave evaluates those tiles, each
//     once: the walk then starts with a best near the final one, and the tiles behind the first surface are skipped.  A tile that is
//     evaluated is copied to LDS, 12 KiB, and read back three words per face, every lane the same address: a broadcast.  The winner
//     is the lexicographic minimum of (t, face) over the hits, so neither the order of the visits nor the skipped tiles change it;
//     its weights and facing are evaluated once more after the walk.
//   No float atomics, no scratch, no workgroup that waits on another.  `evaluated`, where given, takes one integer add per wave.
//
// Bounds.  The workspace holds md_tiles(F) boxes and md_tiles(F) * kMdTile faces of corners, every one written by the boxes launch: a
// tile copy reads whole tiles.  A lane past the last ray reads no ray, reaches no tile and writes nothing; a winner is a loop index
// below F.
#include "common.h"
#include "raycast.h"

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

__device__ __forceinline__ void rc_eval_tile(const RcArgs& a, int t, MdCorner* tile, const RcRay& ray, float& best, int32_t& best_face) {
    const f32x4* __restrict__ from = reinterpret_cast<const f32x4*>(a.corners + (int64_t)t * kMdTile * 3);
    f32x4* to = reinterpret_cast<f32x4*>(tile);
    __syncthreads();          // the tile before has been read
#pragma unroll
    for (int k = 0; k < kMdTile * 3 / kRcThreads; ++k) to[k * kRcThreads + threadIdx.x] = from[k * kRcThreads + threadIdx.x];
    __syncthreads();
    const int64_t left = a.F - (int64_t)t * kMdTile;
    const int count = left < kMdTile ? (int)left : kMdTile;
    const int base = t * kMdTile;
#pragma unroll 2
    for (int j = 0; j < count; ++j) {
        const MdCorner ca = tile[3 * j], cb = tile[3 * j + 1], cc = tile[3 * j + 2];
        const float fa[3] = {ca.x, ca.y, ca.z}, fb[3] = {cb.x, cb.y, cb.z}, fc[3] = {cc.x, cc.y, cc.z};
        const RcPair p = rc_pair(ray, fa, fb, fc);
        const bool better = p.inside && rc_hit(p.t, a.t_min, a.t_max) && rc_better(p.t, base + j, best, best_face);
        best = better ? p.t : best;
        best_face = better ? base + j : best_face;
    }
}

template <bool CULL>
__global__ __launch_bounds__(kRcThreads) void rc_query_kernel(RcArgs a) {
    __shared__ MdCorner tile[kMdTile * 3];
    const int64_t i = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
    const bool own = i < a.R;
    const float nan = bits_float(0x7fc00000u), inf = bits_float(kMdInfBits);
    float o[3], d[3];
    for (int k = 0; k < 3; ++k) o[k] = own ? a.origins[i * 3 + k] : nan, d[k] = own ? a.directions[i * 3 + k] : nan;
    const RcRay ray = rc_ray(o, d);          // a lane past the last ray: not valid, reaches nothing
    const int tiles = (int)md_tiles(a.F);
    float best = inf;
    int32_t best_face = -1;
    unsigned evaluated = 0;
    int nearest = -1;
    if (CULL) {
        float least = inf;
        for (int t0 = 0; t0 < tiles; t0 += kRcScan) {
            float enter[kRcScan];
            bool reach[kRcScan];
#pragma unroll
            for (int k = 0; k < kRcScan; ++k) reach[k] = rc_reach(ray, a.boxes[min(t0 + k, tiles - 1)], a.t_min, a.t_max, &enter[k]);
#pragma unroll
            for (int k = 0; k < kRcScan; ++k) {
                const bool nearer = reach[k] & (t0 + k < tiles) & (enter[k] < least);
                least = nearer ? enter[k] : least;
                nearest = nearer ? t0 + k : nearest;
            }
        }
        unsigned long long pending = __ballot(nearest >= 0);
        while (pending != 0) {          // wave-uniform: at most one trip per lane
            const int t = __builtin_amdgcn_readlane(nearest, __ffsll(pending) - 1);
            rc_eval_tile(a, t, tile, ray, best, best_face);
            evaluated += 1;
            pending &= ~__ballot(nearest == t);
        }
    }
    for (int t0 = 0; t0 < tiles; t0 += kRcScan) {
        bool reach[kRcScan];
        if (CULL) {
            const float to = best < a.t_max ? best : a.t_max;
#pragma unroll
            for (int k = 0; k < kRcScan; ++k) {
                float enter;
                reach[k] = rc_reach(ray, a.boxes[min(t0 + k, tiles - 1)], a.t_min, to, &enter);
            }
        }
#pragma unroll
        for (int k = 0; k < kRcScan; ++k) {
            const int t = t0 + k;
            if (t >= tiles) break;
            if (CULL) {
                // `reach` was taken with the best of the scan's start: a best that has shrunk since only makes it ask for more
                if (__ballot(reach[k]) == 0) continue;
                if (__ballot(nearest == t) != 0) continue;          // evaluated before the walk
            }
            rc_eval_tile(a, t, tile, ray, best, best_face);
            evaluated += 1;
        }
    }
    if (a.evaluated && threadIdx.x == 0 && evaluated) atomicAdd(a.evaluated, (unsigned long long)evaluated);
    if (!own) return;
    float t = inf, bary[3] = {0.f, 0.f, 0.f};
    int8_t front = 0;
    if (best_face >= 0) {          // below F: a loop index
        const MdCorner* c = a.corners + (int64_t)best_face * 3;
        const float fa[3] = {c[0].x, c[0].y, c[0].z}, fb[3] = {c[1].x, c[1].y, c[1].z}, fc[3] = {c[2].x, c[2].y, c[2].z};
        const RcPair p = rc_pair(ray, fa, fb, fc);
        t = p.t;
        rc_finish(p, bary, &front);
    }
    a.t[i] = t;
    a.face[i] = best_face;
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
    const int64_t tiles = md_tiles(F);
    const MdBox* boxes = static_cast<const MdBox*>(ws);          // the layout of md_ws_layout (mesh_distance.hip): boxes, then corners
    const MdCorner* corners = reinterpret_cast<const MdCorner*>(boxes + tiles);
    const RcArgs a{origins, directions, boxes, corners, t, bary, face, front, reinterpret_cast<unsigned long long*>(evaluated), R, F, t_min, t_max};
    const dim3 grid(blocks_for(R, kRcThreads)), block(kRcThreads);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (cull)
        hipLaunchKernelGGL(rc_query_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(rc_query_kernel<false>, grid, block, 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
