// What the point-cloud kernels share (fps.hip, chamfer.hip, emd.hip): the distance expression of their specs, the
// length clamp, and the arguments, limits and launch shape of the two all-pairs directed entry points.
#pragma once
#include "common.h"

namespace npcd {

// The squared distance of the specs, ((dx dx + dy dy) + dz dz) on direct differences, in fp32 as written.  The kernels are held to a
// numpy fp32 evaluation of this expression bit for bit, so EVERY file that includes this header is compiled with -ffp-contract=off
// (csrc/build.py): contracted into fused multiply-adds the products would not be rounded and the low bits would differ.
__device__ __forceinline__ float cloud_sqdist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// valid rows of cloud i: len[i] clamped to [1, full], `full` when len is NULL
__device__ __forceinline__ int cloud_len(const int32_t* len, int i, int full) { return len ? min(max(len[i], 1), full) : full; }

// ---- the all-pairs directed operators: out[i, j] from X cloud i and Y cloud j; a workgroup walks a chunk of Y clouds -----------------
struct CloudPairArgs {
    const float *x, *y;              // [M, P, 3], [N, Q, 3]
    const int32_t *x_len, *y_len;    // [M], [N], either may be NULL
    float* out;                      // [M, N]
    int M, P, N, Q;
    int chunk, nchunks;              // Y clouds per workgroup, workgroups per X cloud (or group of X clouds)
};

constexpr int kCloudPairThreads = 256;
constexpr int kCloudPairMaxClouds = 16384;        // M and N
constexpr int kCloudPairChunk = 32;               // Y clouds per workgroup, at most
constexpr int kCloudPairFill = 2048;              // the chunk shrinks until the grid has this many workgroups
// the grid is one-dimensional: the largest one, one X cloud per workgroup and whole chunks, stays below 2^32 threads
static_assert((int64_t)kCloudPairMaxClouds * (kCloudPairMaxClouds / kCloudPairChunk) * kCloudPairThreads < (int64_t)1 << 32, "grid too large");

// unsupported shape before null pointer
static inline int cloud_pair_check(const float* x, const float* y, const float* out, int M, int P, int N, int Q, int max_points) {
    if (M <= 0 || N <= 0 || P <= 0 || Q <= 0 || P > max_points || Q > max_points || M > kCloudPairMaxClouds || N > kCloudPairMaxClouds)
        return NPCD_ERR_UNSUPPORTED;
    if (!x || !y || !out) return NPCD_ERR_ARG;
    return NPCD_OK;
}

// Y clouds per workgroup and workgroups per group, for `groups` groups of X clouds (the grid is groups * nchunks)
static inline void cloud_pair_chunks(int64_t groups, int N, int* chunk, int* nchunks) {
    int c = kCloudPairChunk;
    while (c > 1 && groups * ((N + c - 1) / c) < kCloudPairFill) c /= 2;
    *chunk = c;
    *nchunks = (N + c - 1) / c;
}

}  // namespace npcd
