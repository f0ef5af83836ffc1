// The walk of one wave over the tiles of a mesh, which md_query_kernel (mesh_distance.hip), rc_query_kernel
// (raycast.hip) and cr_query_kernel (crossings.hip) share; csrc/host_lanes.h is the same walk on the host.  Device only.  A workgroup
// is one wave of Query::kLanes lanes, a lane owns one query with its running Query::State, and its Query judges.  All of them:
//   q.face(c, f, &state)    face f of corners c [3] joins the lane's state
// tile_walk, for a state that is a TileWinner (best, face) whose best shrinks what the lane needs (MdQuery of mesh_distance.h, RcQuery
// of raycast.h):
//   q.rank(box, &value)     the value that ranks the box in the nearest-first pass, the smallest first -> whether the box counts there
//   q.recall(box, best)     what the lane remembers of the box from the start of a scan group of Query::kScan boxes
//   q.needs(memo, best)     whether the lane still needs the tile, given that and its best now
// tile_sweep, for a state that starts as zeros and a need that never shrinks (CrQuery of raycast.h): no nearest-first pass, one test
// per (lane, tile):
//   q.reaches(box)          whether the lane needs the tile
// Barriers.  tile_eval holds two, so every branch around it must be wave-uniform: here each is a loop bound or comes from a __ballot,
// and the workgroup is one wave.  A lane without a query walks with its wave all the same.
// Bounds.  The workspace holds md_tiles(F) boxes and md_tiles(F) * kMdTile faces of corners, every one written by the boxes launch: a
// tile copy reads whole tiles, and a box index is held below md_tiles(F).  A winner is a loop index below F.
#pragma once
#include "common.h"
#include "mesh_tiles.h"

namespace npcd {

// the wave copies tile t to LDS and every lane takes its faces, those below F
template <class Query>
__device__ __forceinline__ void tile_eval(const MdCorner* __restrict__ corners, int64_t F, int t, MdCorner* tile, const Query& q,
                                          typename Query::State& state) {
    const f32x4* __restrict__ from = reinterpret_cast<const f32x4*>(corners + (int64_t)t * kMdTile * 3);
    f32x4* to = reinterpret_cast<f32x4*>(tile);
    __syncthreads();          // the tile before has been read
#pragma unroll
    for (int k = 0; k < kMdTile * 3 / Query::kLanes; ++k) to[k * Query::kLanes + threadIdx.x] = from[k * Query::kLanes + threadIdx.x];
    __syncthreads();
    const int64_t left = F - (int64_t)t * kMdTile;
    const int count = left < kMdTile ? (int)left : kMdTile;
    const int base = t * kMdTile;
    // one face after the other: a state that is a sum would otherwise have the loop vectoriser lay many faces side by side in registers
#pragma clang loop vectorize(disable)
#pragma unroll 2
    for (int j = 0; j < count; ++j) q.face(tile + 3 * j, base + j, &state);
}

// -> the lane's winner; `evaluated`, where given, takes the tiles the wave evaluated: one integer add per wave
template <class Query, bool CULL>
__device__ __forceinline__ TileWinner tile_walk(const Query& q, const MdBox* __restrict__ boxes, const MdCorner* __restrict__ corners, int64_t F,
                                                unsigned long long* evaluated) {
    constexpr int kScan = Query::kScan;
    __shared__ MdCorner tile[kMdTile * 3];
    const int tiles = (int)md_tiles(F);
    TileWinner won{bits_float(kMdInfBits), -1};
    unsigned count = 0;
    int nearest = -1;
    if (CULL) {
        // every lane's box that ranks first, the lowest such, is evaluated before the walk, each tile once: the lane would need it anyway,
        // and the walk then starts with a best that is near the final one (docs/experiments.md R35.1)
        float least = bits_float(kMdInfBits);
        for (int t0 = 0; t0 < tiles; t0 += kScan) {
            float value[kScan];
            bool counts[kScan];
#pragma unroll
            for (int k = 0; k < kScan; ++k) counts[k] = q.rank(boxes[min(t0 + k, tiles - 1)], &value[k]);
#pragma unroll
            for (int k = 0; k < kScan; ++k) {
                const bool nearer = counts[k] & (t0 + k < tiles) & (value[k] < least);
                least = nearer ? value[k] : least;
                nearest = nearer ? t0 + k : nearest;
            }
        }
        unsigned long long pending = __ballot(nearest >= 0);
        while (pending != 0) {          // wave-uniform: at most one trip per lane
            const int t = __builtin_amdgcn_readlane(nearest, __ffsll(pending) - 1);
            tile_eval(corners, F, t, tile, q, won);
            count += 1;
            pending &= ~__ballot(nearest == t);
        }
    }
    for (int t0 = 0; t0 < tiles; t0 += kScan) {          // the boxes through wave-uniform addresses, kScan loads in flight together
        typename Query::Memo memo[kScan];
        if (CULL) {
#pragma unroll
            for (int k = 0; k < kScan; ++k) memo[k] = q.recall(boxes[min(t0 + k, tiles - 1)], won.best);
        }
#pragma unroll
        for (int k = 0; k < kScan; ++k) {
            const int t = t0 + k;
            if (t >= tiles) break;
            if (CULL) {
                if (__ballot(q.needs(memo[k], won.best)) == 0) continue;
                if (__ballot(nearest == t) != 0) continue;          // evaluated before the walk
            }
            tile_eval(corners, F, t, tile, q, won);
            count += 1;
        }
    }
    if (evaluated && threadIdx.x == 0 && count) atomicAdd(evaluated, (unsigned long long)count);
    return won;
}

// -> the lane's state over every tile that some lane of the wave reaches, with CULL, or over all tiles; `evaluated` as above
template <class Query, bool CULL>
__device__ __forceinline__ typename Query::State tile_sweep(const Query& q, const MdBox* __restrict__ boxes, const MdCorner* __restrict__ corners,
                                                            int64_t F, unsigned long long* evaluated) {
    constexpr int kScan = Query::kScan;
    __shared__ MdCorner tile[kMdTile * 3];
    const int tiles = (int)md_tiles(F);
    typename Query::State state{};
    unsigned count = 0;
    for (int t0 = 0; t0 < tiles; t0 += kScan) {
        bool reach[kScan];
        if (CULL) {
#pragma unroll
            for (int k = 0; k < kScan; ++k) reach[k] = q.reaches(boxes[min(t0 + k, tiles - 1)]);
        }
#pragma unroll
        for (int k = 0; k < kScan; ++k) {
            const int t = t0 + k;
            if (t >= tiles) break;
            if (CULL && __ballot(reach[k]) == 0) continue;
            tile_eval(corners, F, t, tile, q, state);
            count += 1;
        }
    }
    if (evaluated && threadIdx.x == 0 && count) atomicAdd(evaluated, (unsigned long long)count);
    return state;
}

}  // namespace npcd
