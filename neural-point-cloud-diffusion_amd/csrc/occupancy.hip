// Occupancy grid of point clouds: every point of every cloud goes to the nearest VALID cell of an R^3 lattice, and two
// integer histograms are taken -- points per cell, and clouds with at least one point in the cell.  The operator under the
// Jensen-Shannon divergence and the occupancy entropy of npcd/eval/shapes.py.
//
//   points [n, P, 3] fp32, lengths [n] or NULL (clamped to [1, P]); lattice g[R] fp32, the same table on the three axes;
//   the valid cells as data: per column (i, j) the inclusive range [k_lo, k_hi] of valid k, k_lo > k_hi an empty column
//   cell(i, j, k) = (i R + j) R + k;  counts[cell] += points, clouds[cell] += clouds that touch it, cells[n, P] = the point's cell
//   or -1 (row at or after the length, non-finite coordinate)
//
// Assignment.  Per axis the nearest lattice index: (v - g[0]) (R - 1) / (g[R-1] - g[0]), clamped to [0, R - 2] and truncated, names
// two neighbours a, a + 1, and the nearer one by direct difference |v - g[.]| is taken -- the division only has to land within one
// cell, so its rounding never decides.  The three indices are the unconstrained nearest cell; if it is valid it is the answer (a
// minimum over a superset).  Otherwise the valid cells are searched exactly: in column (i, j) the best k is the per-axis index
// clamped to [k_lo, k_hi], because the distance along z is monotone on either side of it, so a point costs R^2 candidates.  The
// columns are split over the 64 lanes of the point's wave, candidate distances are cloud_sqdist of clouds.h on direct differences,
// and the wave takes the minimum of (distance bits, cell) keys -- among equal fp32 distances the lowest cell.  One point at a
// time per wave, the points that need it found by a ballot: the search is wave-uniform and no lane idles while others search.
//
// Launch.  1,024 lanes per workgroup, which owns `per_group` consecutive clouds and walks them `teams` at a time: a team is
// 1,024 / teams lanes (whole waves; 16 teams for clouds of up to 64 points, one team from 513 points on) and owns one cloud per
// round.  LDS holds one word per cell, points in the low and clouds in the high 16 bits; one bitmap of R^3 bits per team, the cells
// its cloud has touched; the column table (k_lo, k_hi, i, j in a word) and the lattice.  A point is two LDS atomics: an OR on the
// bitmap, whose returned word says whether the cloud is new to the cell, and one add of 1 or of 0x10001 on the cell's word.  The
// words go to global memory as integer atomics when the workgroup is done, one per touched cell and output, and earlier whenever
// 65,535 points could have gathered in one word.  Bitmaps are cleared between rounds.  No float atomics, no scratch; integer
// sums do not depend on the order of arrival: the same bits on every run.
// The grid aims at one workgroup per compute unit (256; a workgroup takes all the LDS that a unit can give at R = 28): measured,
// the kernel's time follows the number of workgroup rounds, not the arithmetic or the atomics (docs/experiments.md R19.1).
//
// Bounds.  Every index is formed from clamped values: the axis index lies in [0, R - 1] for any finite coordinate (NaN from a
// degenerate lattice clamps to 0), k_hi is clamped to R - 1 when the column table is staged, an empty mask leaves the search key at
// all ones = cell -1, and only cells in [0, R^3) reach an LDS word.  Rows at or after the length are not read.
#include "clouds.h"

namespace npcd {

constexpr int kOccThreads = 1024, kOccMaxTeams = kOccThreads / kWave;
constexpr int kOccMaxResolution = 32;
constexpr int kOccFlushPoints = 0xffff;             // what the low half of a cell's word holds
constexpr int kOccMaxCloudsPerGroup = 4096;         // and this stays far inside the high half
constexpr int kOccFill = 256;                       // workgroups aimed at: one per compute unit, all the LDS of one allows at R = 28
constexpr size_t kOccLdsLimit = 160 * 1024;

struct OccArgs {
    const float* pts;                // [n, P, 3]
    const int32_t* len;              // [n] or NULL
    const float* lattice;            // [R]
    const uint8_t *k_lo, *k_hi;      // [R * R]
    int32_t *counts, *clouds, *cells;          // [R^3], [R^3], [n, P] or NULL
    int n, P, R;
    int teams, per_group;            // clouds walked at a time, clouds per workgroup (a multiple of teams)
};

// dynamic LDS: the cells' words, the column table, the lattice (32 floats), one bitmap per team
static inline size_t occ_lds_bytes(int R, int teams) {
    const size_t cells = (size_t)R * R * R;
    return 4 * (cells + (size_t)R * R + 32 + teams * ((cells + 31) / 32));
}

// teams and clouds per workgroup for n clouds of P points
static inline void occ_shape(int n, int P, int R, int* teams, int* per_group) {
    int t = kOccMaxTeams;
    while (t > 1 && (kOccThreads / t < P || t > n || occ_lds_bytes(R, t) > kOccLdsLimit)) t /= 2;
    const int64_t rounds = ((int64_t)n + (int64_t)t * kOccFill - 1) / ((int64_t)t * kOccFill);
    *teams = t;
    *per_group = (int)(rounds * t < kOccMaxCloudsPerGroup ? rounds * t : kOccMaxCloudsPerGroup);
}

static inline int occ_check(int n, int P, int R) {
    if (n <= 0 || P <= 0 || (int64_t)n * P >= (int64_t)1 << 31 || R < 2 || R > kOccMaxResolution) return NPCD_ERR_UNSUPPORTED;
    return NPCD_OK;
}

// nearest lattice index of one coordinate, always in [0, R - 1]
__device__ __forceinline__ int occ_axis(float v, const float* __restrict__ g, float g0, float inv, int R) {
    const float t = fminf(fmaxf((v - g0) * inv, 0.f), (float)(R - 2));          // fmaxf drops a NaN
    const int a = (int)t;
    return fabsf(v - g[a + 1]) < fabsf(v - g[a]) ? a + 1 : a;
}

// the cells' words into the two outputs, and zero again; between two barriers of its own
__device__ __forceinline__ void occ_flush(uint32_t* __restrict__ hist, int R3, int32_t* __restrict__ counts, int32_t* __restrict__ clouds,
                                          int tid) {
    __syncthreads();
    for (int w = tid; w < R3; w += kOccThreads) {
        const uint32_t v = hist[w];
        if (v) {
            hist[w] = 0;
            atomicAdd(counts + w, (int)(v & 0xffffu));
            if (v >> 16) atomicAdd(clouds + w, (int)(v >> 16));
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kOccThreads) void occupancy_kernel(OccArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t occ_lds[];
    const int R = a.R, R2 = R * R, R3 = R2 * R, words = (R3 + 31) >> 5;
    uint32_t* const hist = occ_lds;                                  // [R3] points | clouds << 16
    uint32_t* const col = hist + R3;                                 // [R2] k_lo | k_hi << 8 | i << 16 | j << 24
    float* const g = reinterpret_cast<float*>(col + R2);             // [32]
    uint32_t* const bits = reinterpret_cast<uint32_t*>(g + 32);      // [teams, words]
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int tt = kOccThreads / a.teams, team = tid / tt, t = tid - team * tt;          // a team is whole waves
    uint32_t* const mine = bits + team * words;

    for (int w = tid; w < R3; w += kOccThreads) hist[w] = 0;
    for (int c = tid; c < R2; c += kOccThreads) {
        const int i = c / R, j = c - i * R;
        int lo = a.k_lo[c], hi = min((int)a.k_hi[c], R - 1);
        if (lo > hi) lo = 1, hi = 0;
        col[c] = (uint32_t)lo | (uint32_t)hi << 8 | (uint32_t)i << 16 | (uint32_t)j << 24;
    }
    if (tid < 32) g[tid] = a.lattice[min(tid, R - 1)];
    const float g0 = a.lattice[0], inv = (float)(R - 1) / (a.lattice[R - 1] - g0);

    const int c0 = blockIdx.x * a.per_group, c1 = min(c0 + a.per_group, a.n);          // c0 < n by the grid's size
    int pending = 0;          // an upper bound of the points added to any word since it was last zero; workgroup-uniform
    for (int cb = c0; cb < c1; cb += a.teams) {
        __syncthreads();          // the tables are staged; nobody is in the round before any more
        for (int w = tid; w < a.teams * words; w += kOccThreads) bits[w] = 0;
        __syncthreads();
        const int cloud = cb + team;
        const bool owns = cloud < c1;
        const int L = owns ? cloud_len(a.len, cloud, a.P) : 0;
        for (int64_t base = 0; base < a.P; base += tt) {          // 64 bits: base + tt may pass 2^31
            if (pending + kOccThreads > kOccFlushPoints) {
                occ_flush(hist, R3, a.counts, a.clouds, tid);
                pending = 0;
            }
            pending += kOccThreads;
            const int64_t p = base + t;
            float x = 0.f, y = 0.f, z = 0.f;
            int cell = -1, iz = 0;
            bool search = false;
            if (p < L) {
                const float* q = a.pts + ((int64_t)cloud * a.P + p) * 3;
                x = q[0], y = q[1], z = q[2];
                if (fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY) {
                    const int column = occ_axis(x, g, g0, inv, R) * R + occ_axis(y, g, g0, inv, R);
                    iz = occ_axis(z, g, g0, inv, R);
                    const uint32_t w = col[column];
                    if (iz >= (int)(w & 0xff) && iz <= (int)(w >> 8 & 0xff)) cell = column * R + iz;
                    else search = true;
                }
            }
            // the points whose unconstrained cell is not valid, one at a time, the columns over the wave's lanes
            for (uint64_t need = __ballot(search); need; need &= need - 1) {
                const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(need));
                const float px = read_lane(x, src), py = read_lane(y, src), pz = read_lane(z, src);
                const int kz = __builtin_amdgcn_readlane(iz, src);
                uint64_t best = ~(uint64_t)0;
                for (int c = lane; c < R2; c += kWave) {
                    const uint32_t w = col[c];
                    const int lo = w & 0xff, hi = w >> 8 & 0xff;
                    if (lo <= hi) {
                        const int k = min(max(kz, lo), hi);
                        const float d = cloud_sqdist(px, py, pz, g[w >> 16 & 0xff], g[w >> 24], g[k]);
                        const uint64_t key = (uint64_t)__float_as_uint(d) << 32 | (uint32_t)(c * R + k);
                        best = key < best ? key : best;
                    }
                }
                best = ~wave_max_u64(~best);          // the smallest key of the wave; all ones when no cell is valid
                if (lane == src) cell = (int)(uint32_t)best;
            }
            if ((uint32_t)cell < (uint32_t)R3) {
                const uint32_t bit = 1u << (cell & 31);
                const uint32_t old = atomicOr(&mine[cell >> 5], bit);
                atomicAdd(&hist[cell], old & bit ? 1u : 0x10001u);
            } else {
                cell = -1;
            }
            if (a.cells && owns && p < a.P) a.cells[(int64_t)cloud * a.P + p] = cell;
        }
    }
    occ_flush(hist, R3, a.counts, a.clouds, tid);
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_occupancy_max_resolution(void) { return kOccMaxResolution; }

extern "C" int npcd_occupancy_clouds_per_workgroup(int n, int P, int R) {
    const int rc = occ_check(n, P, R);
    if (rc != NPCD_OK) return rc;
    int teams, per_group;
    occ_shape(n, P, R, &teams, &per_group);
    return per_group;
}

extern "C" int npcd_occupancy_grid(const float* points, const int32_t* lengths, const float* lattice, const uint8_t* k_lo,
                                   const uint8_t* k_hi, int32_t* counts, int32_t* clouds, int32_t* cells, int n, int P, int R,
                                   void* stream) {
    const int rc = occ_check(n, P, R);
    if (rc != NPCD_OK) return rc;
    if (!points || !lattice || !k_lo || !k_hi || !counts || !clouds) return NPCD_ERR_ARG;
    OccArgs a{points, lengths, lattice, k_lo, k_hi, counts, clouds, cells, n, P, R, 0, 0};
    occ_shape(n, P, R, &a.teams, &a.per_group);
    static DynLds attr;
    const size_t lds = occ_lds_bytes(R, a.teams);
    NPCD_HIP_CHECK(attr.ensure(reinterpret_cast<const void*>(occupancy_kernel), lds));
    hipLaunchKernelGGL(occupancy_kernel, dim3((unsigned)((n + a.per_group - 1) / a.per_group)), dim3(kOccThreads), lds, static_cast<hipStream_t>(stream), a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
