// Bit helpers of the mesh operators (surface.h, simplify.h, smooth.h, mesh_distance.h, components.h), written once for the device and
// the host: the exact-integer forms those operators rest on -- maxima taken on the bits of floats, powers of two made from an
// exponent, floor(log2) read from one.  This header includes nothing of HIP.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define NPCD_HD __host__ __device__ __forceinline__
#else
#define NPCD_HD inline
#endif

namespace npcd {

NPCD_HD uint32_t float_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
NPCD_HD float bits_float(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}
// 2^k as a float64, k in [-1022, 1023]
NPCD_HD double pow2(int k) {
    const uint64_t u = (uint64_t)(k + 1023) << 52;
    double x;
    memcpy(&x, &u, 8);
    return x;
}
NPCD_HD bool is_finite(float x) { return (float_bits(x) & 0x7fffffffu) < 0x7f800000u; }
// the bits of |x| for an integer maximum (x >= +0 orders as its bits do); 0 for a value that is not finite
NPCD_HD uint32_t finite_abs_bits(float x) {
    const uint32_t m = float_bits(x) & 0x7fffffffu;
    return m < 0x7f800000u ? m : 0u;
}
// floor(log2 x) for a finite x > 0, from the exponent of float64(x) (denormals included: float64 holds every float as a normal
// number): -149 .. 127
NPCD_HD int floor_log2(float x) {
    const double d = (double)x;
    uint64_t u;
    memcpy(&u, &d, 8);
    return (int)((u >> 52) & 0x7ff) - 1023;
}
NPCD_HD int popcount32(uint32_t w) {
    w = w - ((w >> 1) & 0x55555555u);
    w = (w & 0x33333333u) + ((w >> 2) & 0x33333333u);
    return (int)((((w + (w >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24);
}

}  // namespace npcd
