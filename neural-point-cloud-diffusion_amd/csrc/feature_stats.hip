// Feature statistics of the diffusion evaluation: the moments behind the Frechet distance and the cubic-kernel
// subset sums behind the kernel inception distance, on the float64 matrix instruction v_mfma_f64_16x16x4_f64.  The operators under
// npcd.hip.feature_stats and npcd.utils.fidkid.DeviceFIDKID.
//
//   moment update   rows [r0, r1) of X [N, D] (fp32 or fp64, row stride ld, unit column stride), optional shift s [D] (float64):
//                     sum[j] += SUM_r (x_rj - s_j);   gram[i][j] += SUM_r (x_ri - s_i)(x_rj - s_j)  for tile(j) >= tile(i)
//   moment finish   mean = s + sum / n;   cov[i][j] = cov[j][i] = (gram[i][j] - n m_i m_j) / (n - 1),  m = sum / n
//   KID subsets     x_i = F[idx_f[s, i]], y_j = R[idx_r[s, j]], k(a, b) = t t t, t = (a . b) / D + 1:
//                     out[s] = (SUM_{i != j} k(x_i, x_j), SUM_{i != j} k(y_i, y_j), SUM_{i, j} k(x_i, y_j))
//
// All arithmetic is float64 (an fp32 feature converts exactly); the epilogues are evaluated as written (no contraction), the products
// and their sums over four k are the matrix instruction's.
//
// The instruction.  Lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one float64 each, and holds four
// results: register g is C[row = (l >> 4) + 4 g][col = l & 15].  (NOT the fp32 map, whose rows are 4 (l >> 4) + g.)
//
// Moments.  A workgroup of 4 waves owns one 64 x 64 block of gram with block(j) >= block(i); a wave owns 32 x 32 of it as 2 x 2
// instructions.  For X^T X both operands are plain row-major reads of X: A = X[r + (l >> 4)][i0 + (l & 15)], B the same at j0, four
// rows per instruction, straight from global memory (16 consecutive features of a row per 16 lanes; the loop is bound by the matrix
// pipe: 4 loads against 4 instructions of 16 passes).  The loads of the next 16 rows are issued before the instructions of this 16.
// Masks are applied to the bits of a loaded value, never as a select on it (the compiler turns that into a branch around the load).
// Rows are added in increasing r; a masked operand (row >= r1, feature >= D) is an exact zero, read from a clamped, valid address.
// The diagonal blocks also sum their 64 columns from the A operands (four partial sums by r mod 4, added in that order).
// Every accumulator element belongs to one lane of one workgroup: gram = gram + acc at the end, no atomics, no fence.
//
// KID.  A workgroup owns one 64 x 64 tile of one of the three kernel matrices of one subset: the tiles on or above the diagonal of
// x x^T and y y^T, all tiles of x y^T.  Per chunk of 32 features it gathers the 64 + 64 rows into LDS as float64 (8 lanes read 32
// consecutive features of a row: coalesced; the next chunk is fetched into registers under this chunk's instructions), pitch 34 doubles, so that the operand read of a half wave (16 rows x 2 k) touches 32
// different bank pairs.  The epilogue forms k, leaves out i == j of the symmetric matrices exactly, sums the tile through the fixed
// tree of wave.h and the four waves in order, doubles an off-diagonal symmetric tile (exact) and writes one workspace slot.  A second
// launch adds the slots of each (subset, matrix) in a fixed order.  No atomics: the same bits on every run.
//
// Bounds.  Feature and row indices are clamped before every load (the mask zeroes the value afterwards); idx entries are validated
// by the caller and clamped to the row count here as well; gram, cov and the workspace are indexed in 64 bits.  35,872 bytes of
// static LDS in the KID tiles kernel, 33,280 in the moment finish, no scratch.
#include "common.h"

namespace npcd {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kFsThreads = 256, kFsWaves = kFsThreads / kWave;
constexpr int kFsTile = 64;                 // a workgroup's square block of gram and of a kernel matrix
constexpr int kFsMaxD = 4096;
constexpr int kFsGroup = 4;                 // instructions along r between two rounds of loads
constexpr int kKidChunk = 32, kKidPitch = kKidChunk + 2;

__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// v, or an exact +0 where the mask is 0 (all ones otherwise)
__device__ __forceinline__ double masked(double v, uint64_t mask) {
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, v) & mask);
}

// block id -> (bi, bj) with bj >= bi, row by row of the upper triangle of nb x nb blocks
__device__ __forceinline__ void upper_block(int bid, int nb, int& bi, int& bj) {
    bi = 0;
    while (bid >= nb - bi) bid -= nb - bi, ++bi;
    bj = bi + bid;
}

static inline int64_t upper_count(int nb) { return (int64_t)nb * (nb + 1) / 2; }

// ---- moments ---------------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kFsThreads) void moments_update_kernel(const T* __restrict__ x, int64_t ld, int64_t r0, int64_t r1, int D,
                                                                    const double* __restrict__ shift, double* __restrict__ sum,
                                                                    double* __restrict__ gram) {
    __shared__ double cs[4][kFsTile];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, wi = wave >> 1, wj = wave & 1;
    const int l15 = lane & 15, kq = lane >> 4;
    int bi, bj;
    upper_block(blockIdx.x, (D + kFsTile - 1) / kFsTile, bi, bj);
    const int i0 = bi * kFsTile + wi * 32, j0 = bj * kFsTile + wj * 32;
    // operands 0, 1: the two A tiles; 2, 3: the two B tiles
    int col[4] = {i0 + l15, i0 + 16 + l15, j0 + l15, j0 + 16 + l15};
    bool ok[4];
    double s[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        ok[o] = col[o] < D;
        col[o] = ok[o] ? col[o] : D - 1;
        s[o] = shift ? shift[col[o]] : 0.0;
    }
    const bool sums = bi == bj && wj == 0;          // wave-uniform: this wave's A operands are 32 columns of the diagonal block
    f64x4 acc[2][2] = {};
    double part[2] = {0.0, 0.0};
    const int64_t last = r1 - 1;

    // every load is issued, from a clamped address, and the mask is applied to the bits of the value: a select on the loaded value
    // is turned into a branch around the load by the compiler, with a full wait behind each
    uint64_t cmask[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) cmask[o] = ok[o] ? ~0ull : 0ull;
    auto load = [&](int64_t r, double (&v)[kFsGroup][4]) {
        T raw[kFsGroup][4];
        uint64_t rmask[kFsGroup];
#pragma unroll
        for (int q = 0; q < kFsGroup; ++q) {
            const int64_t row = r + 4 * q + kq;
            rmask[q] = row < r1 ? ~0ull : 0ull;
            const T* p = x + (row < r1 ? row : last) * ld;
#pragma unroll
            for (int o = 0; o < 4; ++o) raw[q][o] = p[col[o]];
        }
#pragma unroll
        for (int q = 0; q < kFsGroup; ++q)
#pragma unroll
            for (int o = 0; o < 4; ++o) v[q][o] = masked((double)raw[q][o] - s[o], cmask[o] & rmask[q]);
    };
    double cur[kFsGroup][4], nxt[kFsGroup][4];
    load(r0, cur);
    for (int64_t r = r0; r < r1; r += 4 * kFsGroup) {
        load(r + 4 * kFsGroup, nxt);          // past r1 at the end: clamped and masked, never used
#pragma unroll
        for (int q = 0; q < kFsGroup; ++q) {
            acc[0][0] = mfma_f64(cur[q][0], cur[q][2], acc[0][0]);
            acc[0][1] = mfma_f64(cur[q][0], cur[q][3], acc[0][1]);
            acc[1][0] = mfma_f64(cur[q][1], cur[q][2], acc[1][0]);
            acc[1][1] = mfma_f64(cur[q][1], cur[q][3], acc[1][1]);
            if (sums) part[0] += cur[q][0], part[1] += cur[q][1];
        }
#pragma unroll
        for (int q = 0; q < kFsGroup; ++q)
#pragma unroll
            for (int o = 0; o < 4; ++o) cur[q][o] = nxt[q][o];
    }
    // gram = gram + acc: the sixteen old values are read together (clamped addresses), only the stores are masked
    double old[2][2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = min(i0 + 16 * a + kq + 4 * g, D - 1), j = min(j0 + 16 * b + l15, D - 1);
                old[a][b][g] = gram[(int64_t)i * D + j];
            }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = i0 + 16 * a + kq + 4 * g, j = j0 + 16 * b + l15;
                if (i < D && j < D) gram[(int64_t)i * D + j] = old[a][b][g] + acc[a][b][g];
            }
    if (bi == bj) {          // workgroup-uniform
        if (sums) cs[kq][wi * 32 + l15] = part[0], cs[kq][wi * 32 + 16 + l15] = part[1];
        __syncthreads();
        const int c = bi * kFsTile + tid;
        if (tid < kFsTile && c < D) sum[c] = sum[c] + (((cs[0][tid] + cs[1][tid]) + cs[2][tid]) + cs[3][tid]);
    }
}

// one workgroup per 64 x 64 block on or above the diagonal: the block of cov and its mirror image from one computed value
__global__ __launch_bounds__(kFsThreads) void moments_finish_kernel(const double* __restrict__ sum, const double* __restrict__ gram,
                                                                    const double* __restrict__ shift, int D, double n,
                                                                    double* __restrict__ mean, double* __restrict__ cov) {
    __shared__ double t[kFsTile][kFsTile + 1];
    const int tid = threadIdx.x;
    int bi, bj;
    upper_block(blockIdx.x, (D + kFsTile - 1) / kFsTile, bi, bj);
    const int i0 = bi * kFsTile, j0 = bj * kFsTile;
    for (int e = tid; e < kFsTile * kFsTile; e += kFsThreads) {
        const int a = e / kFsTile, b = e % kFsTile, i = i0 + a, j = j0 + b;
        if (i < D && j < D && (bi != bj || b >= a)) {
            const double mi = sum[i] / n, mj = sum[j] / n;
            const double v = (gram[(int64_t)i * D + j] - n * mi * mj) / (n - 1.0);
            t[a][b] = v;
            if (bi == bj) t[b][a] = v;
        }
    }
    __syncthreads();
    for (int e = tid; e < kFsTile * kFsTile; e += kFsThreads) {
        const int a = e / kFsTile, b = e % kFsTile;
        if (i0 + a < D && j0 + b < D) cov[(int64_t)(i0 + a) * D + (j0 + b)] = t[a][b];
        if (bi != bj && j0 + a < D && i0 + b < D) cov[(int64_t)(j0 + a) * D + (i0 + b)] = t[b][a];
    }
    if (bi == bj && tid < kFsTile && i0 + tid < D) {
        const int c = i0 + tid;
        mean[c] = (shift ? shift[c] : 0.0) + sum[c] / n;
    }
}

// ---- KID ---------------------------------------------------------------------------------------------------------------------------------
struct KidArgs {
    const void *f, *r;                 // [Nf, D], [Nr, D]
    int64_t ldf, ldr;
    const int32_t *idx_f, *idx_r;      // [S, m]
    double* ws;                        // [S, per]
    int Nf, Nr, m, D, T, U, per;       // T tiles along m; U = T (T + 1) / 2; per = 2 U + T T slots of a subset
};

template <class T>
__global__ __launch_bounds__(kFsThreads) void kid_tiles_kernel(KidArgs a) {
    __shared__ double sa[kFsTile][kKidPitch], sb[kFsTile][kKidPitch];
    __shared__ const T* rows[2][kFsTile];
    __shared__ double red[kFsWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, wi = wave >> 1, wj = wave & 1;
    const int l15 = lane & 15, kq = lane >> 4;
    const int s = blockIdx.x / a.per;
    int slot = blockIdx.x - s * a.per, which, ti, tj;
    if (slot < 2 * a.U) {
        which = slot >= a.U;
        upper_block(slot - which * a.U, a.T, ti, tj);
    } else {
        which = 2;
        ti = (slot - 2 * a.U) / a.T, tj = (slot - 2 * a.U) % a.T;
    }
    const bool left_f = which != 1, right_f = which == 0;          // x x^T, y y^T, x y^T
    if (tid < 2 * kFsTile) {
        const int side = tid / kFsTile, q = tid % kFsTile;
        const bool from_f = side == 0 ? left_f : right_f;
        const int e = min((side == 0 ? ti : tj) * kFsTile + q, a.m - 1);
        const int32_t* idx = from_f ? a.idx_f : a.idx_r;
        const int row = min(max(idx[(int64_t)s * a.m + e], 0), (from_f ? a.Nf : a.Nr) - 1);
        rows[side][q] = from_f ? (const T*)a.f + row * a.ldf : (const T*)a.r + row * a.ldr;
    }
    __syncthreads();
    f64x4 acc[2][2] = {};
    const int lr = tid >> 3, lc = (tid & 7) * 4;          // staging: 8 lanes take the 32 features of a row, 32 rows per pass
    const T *pa[2] = {rows[0][lr], rows[0][lr + 32]}, *pb[2] = {rows[1][lr], rows[1][lr + 32]};
    T ra[2][4], rb[2][4];
    // the chunk's features of this lane's rows, from clamped addresses; the mask is applied to the bits when they are staged
    auto fetch = [&](int d0) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int d = min(d0 + lc + c, a.D - 1);
                ra[pass][c] = pa[pass][d], rb[pass][c] = pb[pass][d];
            }
    };
    fetch(0);
    for (int d0 = 0; d0 < a.D; d0 += kKidChunk) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint64_t mask = d0 + lc + c < a.D ? ~0ull : 0ull;
                sa[lr + 32 * pass][lc + c] = masked((double)ra[pass][c], mask);
                sb[lr + 32 * pass][lc + c] = masked((double)rb[pass][c], mask);
            }
        __syncthreads();
        fetch(d0 + kKidChunk);          // in flight under the instructions of this chunk; past D at the end: clamped, never staged
#pragma unroll
        for (int k = 0; k < kKidChunk; k += 4) {
            const double a0 = sa[wi * 32 + l15][k + kq], a1 = sa[wi * 32 + 16 + l15][k + kq];
            const double b0 = sb[wj * 32 + l15][k + kq], b1 = sb[wj * 32 + 16 + l15][k + kq];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    const double Dd = (double)a.D;
    double total = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ti * kFsTile + wi * 32 + 16 * p + kq + 4 * g, j = tj * kFsTile + wj * 32 + 16 * q + l15;
                const double t = acc[p][q][g] / Dd + 1.0;
                const double k = t * t * t;
                if (i < a.m && j < a.m && (which == 2 || i != j)) total += k;
            }
    total = wave_sum_tree(total);
    if (lane == 0) red[wave] = total;
    __syncthreads();
    if (tid == 0) {
        const double v = ((red[0] + red[1]) + red[2]) + red[3];
        a.ws[(int64_t)s * a.per + slot] = which != 2 && ti != tj ? 2.0 * v : v;
    }
}

// one workgroup per subset: the slots of each of its three matrices in a fixed order
__global__ __launch_bounds__(kFsThreads) void kid_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int U, int per) {
    __shared__ double red[kFsWaves];
    const int tid = threadIdx.x, s = blockIdx.x;
    const double* slots = ws + (int64_t)s * per;
    for (int w = 0; w < 3; ++w) {
        const int lo = w * U, hi = w == 2 ? per : lo + U;
        double v = 0.0;
        for (int t = lo + tid; t < hi; t += kFsThreads) v += slots[t];
        v = wave_sum_tree(v);
        __syncthreads();          // nobody reads the sums of the matrix before any more
        if ((tid & (kWave - 1)) == 0) red[tid / kWave] = v;
        __syncthreads();
        if (tid == 0) out[3 * (int64_t)s + w] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

static inline int moments_check(int D) { return D < 1 || D > kFsMaxD ? NPCD_ERR_UNSUPPORTED : NPCD_OK; }

static inline int64_t kid_slots(int m) {
    const int64_t T = ceil_div(m, kFsTile);
    return T * (T + 1) + T * T;
}

static inline int kid_check(int S, int m) {
    if (S < 1 || m < 2 || m > (1 << 20)) return NPCD_ERR_UNSUPPORTED;
    return (int64_t)S * kid_slots(m) >= (int64_t)1 << 31 ? NPCD_ERR_UNSUPPORTED : NPCD_OK;
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_moments_tile(int* tile_host) {
    if (!tile_host) return NPCD_ERR_ARG;
    *tile_host = kFsTile;
    return NPCD_OK;
}

extern "C" int npcd_moments_max_features(void) { return kFsMaxD; }

extern "C" int npcd_moments_update(const void* x, int dtype, int64_t ld, int64_t r0, int64_t r1, int D, const double* shift, double* sum,
                                   double* gram, void* stream) {
    const int rc = moments_check(D);
    if (rc != NPCD_OK) return rc;
    if (dtype != NPCD_F32 && dtype != NPCD_F64) return NPCD_ERR_UNSUPPORTED;
    if (!x || !sum || !gram || r0 < 0 || r1 < r0 || ld < D) return NPCD_ERR_ARG;
    if (r1 == r0) return NPCD_OK;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)upper_count(ceil_div(D, kFsTile)));
    if (dtype == NPCD_F32)
        hipLaunchKernelGGL(moments_update_kernel<float>, grid, dim3(kFsThreads), 0, s, (const float*)x, ld, r0, r1, D, shift, sum, gram);
    else
        hipLaunchKernelGGL(moments_update_kernel<double>, grid, dim3(kFsThreads), 0, s, (const double*)x, ld, r0, r1, D, shift, sum, gram);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_moments_finish(const double* sum, const double* gram, const double* shift, int D, int64_t n, double* mean, double* cov,
                                   void* stream) {
    const int rc = moments_check(D);
    if (rc != NPCD_OK) return rc;
    if (n < 2) return NPCD_ERR_UNSUPPORTED;
    if (!sum || !gram || !mean || !cov) return NPCD_ERR_ARG;
    hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)upper_count(ceil_div(D, kFsTile))), dim3(kFsThreads), 0,
                       static_cast<hipStream_t>(stream), sum, gram, shift, D, (double)n, mean, cov);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_kid_tile(int* tile_host) {
    if (!tile_host) return NPCD_ERR_ARG;
    *tile_host = kFsTile;
    return NPCD_OK;
}

extern "C" int64_t npcd_kid_workspace_bytes(int S, int m) {
    const int rc = kid_check(S, m);
    if (rc != NPCD_OK) return rc;
    return (int64_t)S * kid_slots(m) * (int64_t)sizeof(double);
}

extern "C" int npcd_kid_subsets(const void* fake, const void* real, int dtype, int Nf, int Nr, int D, int64_t ldf, int64_t ldr,
                                const int32_t* idx_f, const int32_t* idx_r, int S, int m, double* workspace, double* out, void* stream) {
    int rc = moments_check(D);
    if (rc == NPCD_OK) rc = kid_check(S, m);
    if (rc != NPCD_OK) return rc;
    if (dtype != NPCD_F32 && dtype != NPCD_F64) return NPCD_ERR_UNSUPPORTED;
    if (!fake || !real || !idx_f || !idx_r || !workspace || !out || Nf < 1 || Nr < 1 || ldf < D || ldr < D) return NPCD_ERR_ARG;
    const int T = ceil_div(m, kFsTile), U = T * (T + 1) / 2;
    KidArgs a{fake, real, ldf, ldr, idx_f, idx_r, workspace, Nf, Nr, m, D, T, U, 2 * U + T * T};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((int64_t)S * a.per));
    if (dtype == NPCD_F32)
        hipLaunchKernelGGL(kid_tiles_kernel<float>, grid, dim3(kFsThreads), 0, s, a);
    else
        hipLaunchKernelGGL(kid_tiles_kernel<double>, grid, dim3(kFsThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kid_finish_kernel, dim3((unsigned)S), dim3(kFsThreads), 0, s, workspace, out, U, a.per);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
