// Prefix sums of unsigned integers over a workgroup, on the scan tree of wave.h: the one scan of the mesh kernels (surface.hip,
// simplify.hip, smooth.hip: 256 lanes) and of the isosurface (1,024 lanes).  Integer sums: no result depends on the order of the
// additions.  Workgroups of one dimension; every lane of the workgroup makes every call, the same number of times.
#pragma once
#include "wave.h"

namespace npcd {

// -> the sum of v over lanes 0 .. threadIdx.x -- INCLUSIVE: with the lane's own v, else without --, and to *total the sum over the
// workgroup's LANES lanes.  wave_scan_incl, then the wave totals through wave_total, LDS [LANES / 64], and two barriers: after the
// second the totals may be written again.
template <int LANES, bool INCLUSIVE>
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* wave_total, uint64_t* total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t incl = wave_scan_incl(v, (uint64_t)0, AddU64());
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < LANES / 64; ++w) {
        const uint64_t t = wave_total[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return INCLUSIVE ? before + incl : before + incl - v;
}

// One workgroup turns x [n] into its prefix sums in place, LANES entries at a time, the carry taken from the scan's total; -> the sum
// of all, in every lane.  INCLUSIVE: x[i] becomes the sum up to and including itself, else the sum before it.  T: uint32_t, or
// uint64_t -- also for several counts packed into one word, as long as no field overflows.
template <int LANES, bool INCLUSIVE, class T>
__device__ __forceinline__ uint64_t block_scan_totals(T* x, int64_t n, uint64_t* wave_total) {
    uint64_t carry = 0;
    for (int64_t first = 0; first < n; first += LANES) {          // the same trips for every lane
        const int64_t i = first + threadIdx.x;
        const uint64_t own = i < n ? (uint64_t)x[i] : 0;
        uint64_t total;
        const uint64_t sum = carry + block_scan<LANES, INCLUSIVE>(own, wave_total, &total);
        if (i < n) x[i] = (T)sum;
        carry += total;
    }
    return carry;
}

}  // namespace npcd
