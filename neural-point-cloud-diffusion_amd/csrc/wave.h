// Wave-level reductions on the vector ALU (DPP and lane swaps, no LDS crossbar).  Every kernel that promises "the same bits on every
// run" sums through one of the two fixed trees below: this file is the only place their DPP controls are written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace npcd {

// ---- all lanes: every lane ends with op over the 64 lanes ---------------------------------------------------------------------------
// four DPP row rotations inside the 16-lane rows, then v_permlane16_swap and v_permlane32_swap across them -- no ds_bpermute round
// trips.  Fixed order: bitwise reproducible.
template <class Op>
__device__ __forceinline__ float wave_reduce64(float x, Op op) {
    x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128 /* row_ror:8 */, 0xf, 0xf, false)));
    x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124 /* row_ror:4 */, 0xf, 0xf, false)));
    x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x122 /* row_ror:2 */, 0xf, 0xf, false)));
    x = op(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x121 /* row_ror:1 */, 0xf, 0xf, false)));
    const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = op(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
    const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return op(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}
__device__ __forceinline__ float wave_max64(float x) { return wave_reduce64(x, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ float wave_sum64(float x) { return wave_reduce64(x, [](float a, float b) { return a + b; }); }

// ---- the scan tree: lane l ends with op over lanes 0 .. l, so lane 15 of a row holds the row and lane 63 the wave -------------------
// the value of the lane that CTRL names; a lane without a source, or in a row outside ROWMASK, receives `ident`.  A 64-bit payload
// moves as two 32-bit halves.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_mov(float ident, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ident), __float_as_int(v), CTRL, ROWMASK, 0xf, false));
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint64_t dpp_mov(uint64_t ident, uint64_t v) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(ident >> 32), (int)(uint32_t)(v >> 32), CTRL, ROWMASK, 0xf, false);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)ident, (int)(uint32_t)v, CTRL, ROWMASK, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_mov(double ident, double v) {
    return __builtin_bit_cast(double, dpp_mov<CTRL, ROWMASK>(__builtin_bit_cast(uint64_t, ident), __builtin_bit_cast(uint64_t, v)));
}
template <int CTRL, int ROWMASK, class T, class Op>
__device__ __forceinline__ T dpp_step(T v, T ident, Op op) {
    return op(v, dpp_mov<CTRL, ROWMASK>(ident, v));
}
// inside each 16-lane row
template <class T, class Op>
__device__ __forceinline__ T row_scan_incl(T v, T ident, Op op) {
    v = dpp_step<0x111 /* row_shr:1 */, 0xf>(v, ident, op);
    v = dpp_step<0x112 /* row_shr:2 */, 0xf>(v, ident, op);
    v = dpp_step<0x114 /* row_shr:4 */, 0xf>(v, ident, op);
    v = dpp_step<0x118 /* row_shr:8 */, 0xf>(v, ident, op);
    return v;
}
// over the wave
template <class T, class Op>
__device__ __forceinline__ T wave_scan_incl(T v, T ident, Op op) {
    v = row_scan_incl(v, ident, op);
    v = dpp_step<0x142 /* row_bcast:15 */, 0xa>(v, ident, op);     // rows 1 and 3 take the total of the row before them
    v = dpp_step<0x143 /* row_bcast:31 */, 0xc>(v, ident, op);     // rows 2 and 3 take the total of rows 0-1
    return v;
}

__device__ __forceinline__ float read_lane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ uint64_t read_lane(uint64_t v, int lane) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    return ((uint64_t)hi << 32) | lo;
}

// sum over the wave in that one fixed tree, wave-uniform (read from lane 63); lanes without a source, or outside the row mask, add 0
__device__ __forceinline__ float wave_sum_tree(float v) {
    return read_lane(wave_scan_incl(v, 0.f, [](float a, float b) { return a + b; }), 63);
}
// the same tree on float64 (csrc/ssim.hip)
__device__ __forceinline__ double wave_sum_tree(double v) {
    const double s = wave_scan_incl(v, 0.0, [](double a, double b) { return a + b; });
    return __builtin_bit_cast(double, read_lane(__builtin_bit_cast(uint64_t, s), 63));
}
// maximum of unsigned keys: over the 16 lanes of each row, in the row's lane 15; and over the wave, wave-uniform.  Lanes without a
// source keep their own value: the identity is key 0
struct MaxU64 {
    __device__ __forceinline__ uint64_t operator()(uint64_t v, uint64_t o) const { return o > v ? o : v; }
};
__device__ __forceinline__ uint64_t row_max_u64(uint64_t v) { return row_scan_incl(v, (uint64_t)0, MaxU64()); }
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) { return read_lane(wave_scan_incl(v, (uint64_t)0, MaxU64()), 63); }
// integer sums: the prefix sums of csrc/block_scan.h
struct AddU64 {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};

// the maximum of `bits` over the wave into *target, a word that only grows: lane 0 reads it first and issues the one atomic only if
// the wave's maximum is larger.  A maximum does not depend on how often or in what order it is applied.  Every lane of the wave
// calls it (workgroups of one dimension).
__device__ __forceinline__ void wave_publish_max(uint32_t bits, uint32_t* target) {
    const uint32_t top = (uint32_t)wave_max_u64(bits);
    if ((threadIdx.x & 63) == 0 && top > __hip_atomic_load(target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_max(target, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace npcd
