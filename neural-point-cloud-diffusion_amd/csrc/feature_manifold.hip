// Feature k-NN of the diffusion evaluation: the k smallest squared distances of every row of one feature set to
// another, and the ball counts behind improved precision / recall and density / coverage, on the float64 matrix instruction
// v_mfma_f64_16x16x4_f64.  The operators under npcd.hip.feature_manifold and npcd.utils.fidkid.DeviceFIDKID(prdc=True).
//
//   d2_ij = max((nx_i + ny_j) - 2 g_ij, +0),   g_ij = x_i . y_j,   nx_i = x_i . x_i,   ny_j = y_j . y_j      X [n, D], Y [m, D]
//   k-NN          out[i][0 .. k) = the k smallest d2_ij over the j that exist, ascending, equal values kept (a multiset)
//   ball counts   cnt[i] = #{j : d2_ij < rho_y[j]},   near[i] = min_j d2_ij
// Columns j >= m do not exist; with exclude_self the pair j == i does not exist either (by index, whatever its value).
//
// All arithmetic is float64 (an fp32 feature converts exactly); the epilogue is evaluated as written (no contraction), the products
// and their sums over four features are the matrix instruction's.  The lane map of the instruction is in feature_stats.hip's header:
// register g of lane l is C[row = (l >> 4) + 4 g][col = l & 15].
//
// Norms.  One wave per row: lane l squares features l, l + 64, ... and adds them in that order, the 64 partial sums go through the
// fixed tree of wave.h.  A pre-pass into the workspace, so a norm does not depend on which workgroup uses it.
//
// Tiles.  A workgroup of 4 waves owns 64 rows of X and streams a contiguous range of the 64-row tiles of Y; a wave owns 32 x 32 of
// the 64 x 64 distance tile as 2 x 2 instructions.  Per chunk of 32 features both operands are staged into LDS as float64 (8 lanes
// read 32 consecutive features of a row, pitch 34 doubles; the next chunk -- of this tile or the first of the next -- is fetched into
// registers under this chunk's instructions), exactly as kid_tiles_kernel does.  g_ij is therefore accumulated in chunk order, whatever
// the partition of the columns.  The epilogue writes the tile's d2 (+inf where the pair does not exist) into the same LDS, pitch 65,
// and every thread scans 16 columns of one row: wave w takes columns 16 w .. 16 w + 15 of all 64 rows.  A thread keeps the 8 smallest
// values it has seen, ascending, in registers (compare-exchange chain, no indexing by a variable), or a count and a minimum.  After the
// last tile the four threads of a row merge through LDS.  The distance matrix is never stored.
//
// Column splits.  With `splits` > 1 workgroups per row block each takes tiles [s T / splits, (s + 1) T / splits) and writes its
// partial lists (counts, minima) to the workspace; a finish kernel merges the splits of a row in the order s = 0, 1, ...  The k
// smallest of a multiset, a count and a minimum do not depend on the order: the same bits for every `splits` and on every run.  No
// atomics, no fence.
//
// Bounds.  Row and feature indices are clamped before every load and the mask is applied to the bits of the value afterwards; row
// offsets and output indices are 64-bit.  35,840 bytes of static LDS in the tiles kernel (37,376 in the ball form), no scratch.
#include "common.h"

namespace npcd {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kFmThreads = 256, kFmWaves = kFmThreads / kWave;
constexpr int kFmTile = 64;                 // rows of X of a workgroup, rows of Y of a tile
constexpr int kFmMaxD = 4096;
constexpr int kFmMaxK = 8;
constexpr int kFmMaxRows = 1 << 24;
constexpr int kFmMaxSplits = 256;
// automatic splits: some 8,192 workgroups where m allows, eight rounds of the 1,024 that are resident (four on a CU), so that the last,
// partly filled round is a small part of the launch (docs/experiments.md R25.1)
constexpr int kFmTargetGroups = 8192;
constexpr int kFmChunk = 32, kFmPitch = kFmChunk + 2;
constexpr int kFmDistPitch = kFmTile + 1;                    // the scan of a wave reads 64 rows of one column: 64 different bank pairs
constexpr int kFmMergePitch = kFmWaves * kFmMaxK + 1;
static_assert(kFmTile * kFmDistPitch <= 2 * kFmTile * kFmPitch && kFmTile * kFmMergePitch <= 2 * kFmTile * kFmPitch, "the epilogue reuses the staging LDS");

__device__ __forceinline__ f64x4 fm_mfma_f64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// v, or an exact +0 where the mask is 0 (all ones otherwise)
__device__ __forceinline__ double fm_masked(double v, uint64_t mask) {
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, v) & mask);
}

// best: ascending, the 8 smallest so far (+inf where fewer).  Equal values are kept: a multiset.
__device__ __forceinline__ void keep_smallest(double (&best)[kFmMaxK], double v) {
    if (v < best[kFmMaxK - 1]) {
        best[kFmMaxK - 1] = v;
#pragma unroll
        for (int t = kFmMaxK - 1; t > 0; --t) {
            const double lo = best[t - 1], hi = best[t];
            const bool swap = hi < lo;
            best[t - 1] = swap ? hi : lo;
            best[t] = swap ? lo : hi;
        }
    }
}

// ---- row norms ---------------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kFmThreads) void feature_norms_kernel(const T* __restrict__ x, int64_t ld, int n, int D, double* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t row = (int64_t)blockIdx.x * kFmWaves + wave;
    const T* p = x + (row < n ? row : (int64_t)n - 1) * ld;
    double s = 0.0;
    for (int d0 = 0; d0 < D; d0 += kWave) {
        const int d = d0 + lane;
        const double v = fm_masked((double)p[min(d, D - 1)], d < D ? ~0ull : 0ull);
        s += v * v;
    }
    s = wave_sum_tree(s);
    if (lane == 0 && row < n) out[row] = s;
}

// ---- distance tiles ------------------------------------------------------------------------------------------------------------------------
struct RowsArgs {
    const void *x, *y;                 // [n, D], [m, D]
    int64_t ldx, ldy;
    const double *nx, *ny, *rho;       // [n], [m], [m] (ball counts only)
    double* lists;                     // k-NN: [splits, n, k]
    int32_t* cnt;                      // ball counts: [splits, n]
    double* near;                      //              [splits, n]
    int n, m, D, k, splits, tiles, row_blocks, exclude_self;
};

// asked for three waves on a SIMD, the compiler lands at 112-128 registers, all of them VGPRs: four workgroups on a CU, which their
// LDS allows as well.  Without the request it took 144-172 with 32 AGPRs, two to three workgroups (docs/experiments.md R25.1)
template <class T, bool kBall>
__global__ __launch_bounds__(kFmThreads, 3) void feature_rows_kernel(RowsArgs a) {
    __shared__ double smem[2 * kFmTile * kFmPitch];
    __shared__ double nxs[kFmTile], nys[kFmTile];
    __shared__ double rhos[kBall ? kFmTile : 1];
    __shared__ int cnts[kBall ? kFmTile * kFmWaves : 1];
    double(*sa)[kFmPitch] = reinterpret_cast<double(*)[kFmPitch]>(smem);
    double(*sb)[kFmPitch] = sa + kFmTile;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, wi = wave >> 1, wj = wave & 1;
    const int l15 = lane & 15, kq = lane >> 4;
    // neighbouring workgroups take the same tiles of Y for different rows of X
    const int sp = blockIdx.x / a.row_blocks, i0 = (blockIdx.x - sp * a.row_blocks) * kFmTile;
    const int t0 = (int)((int64_t)sp * a.tiles / a.splits), t1 = (int)((int64_t)(sp + 1) * a.tiles / a.splits);

    const int lr = tid >> 3, lc = (tid & 7) * 4;          // staging: 8 lanes take the 32 features of a row, 32 rows per pass
    const T* px[2];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) px[pass] = (const T*)a.x + (int64_t)min(i0 + lr + 32 * pass, a.n - 1) * a.ldx;
    T ra[2][4], rb[2][4];
    // the chunk's features of this lane's rows of X and of tile `tile` of Y, from clamped addresses; the mask is applied to the bits
    // when they are staged
    auto fetch = [&](int tile, int d0) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const T* py = (const T*)a.y + (int64_t)min(tile * kFmTile + lr + 32 * pass, a.m - 1) * a.ldy;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int d = min(d0 + lc + c, a.D - 1);
                ra[pass][c] = px[pass][d], rb[pass][c] = py[d];
            }
        }
    };

    const double inf = __builtin_inf();
    double best[kFmMaxK];
#pragma unroll
    for (int t = 0; t < kFmMaxK; ++t) best[t] = inf;
    int count = 0;
    double nearest = inf;
    const int r = lane, c0 = wave * (kFmTile / kFmWaves);          // the scan: this thread's row and its first column of a tile
    if (tid < kFmTile) nxs[tid] = a.nx[min(i0 + tid, a.n - 1)];
    fetch(t0, 0);
    for (int tile = t0; tile < t1; ++tile) {
        if (tid < kFmTile) {          // read after the barriers of the chunk loop; the last readers are behind the barrier that ends a tile
            const int j = min(tile * kFmTile + tid, a.m - 1);
            nys[tid] = a.ny[j];
            if (kBall) rhos[tid] = a.rho[j];
        }
        f64x4 acc[2][2] = {};
        for (int d0 = 0; d0 < a.D; d0 += kFmChunk) {
#pragma unroll
            for (int pass = 0; pass < 2; ++pass)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint64_t mask = d0 + lc + c < a.D ? ~0ull : 0ull;
                    sa[lr + 32 * pass][lc + c] = fm_masked((double)ra[pass][c], mask);
                    sb[lr + 32 * pass][lc + c] = fm_masked((double)rb[pass][c], mask);
                }
            __syncthreads();
            // in flight under the instructions of this chunk; past the last tile at the end: clamped, never staged
            const bool last = d0 + kFmChunk >= a.D;
            fetch(last ? tile + 1 : tile, last ? 0 : d0 + kFmChunk);
#pragma unroll
            for (int k = 0; k < kFmChunk; k += 4) {
                const double a0 = sa[wi * 32 + l15][k + kq], a1 = sa[wi * 32 + 16 + l15][k + kq];
                const double b0 = sb[wj * 32 + l15][k + kq], b1 = sb[wj * 32 + 16 + l15][k + kq];
                acc[0][0] = fm_mfma_f64(a0, b0, acc[0][0]);
                acc[0][1] = fm_mfma_f64(a0, b1, acc[0][1]);
                acc[1][0] = fm_mfma_f64(a1, b0, acc[1][0]);
                acc[1][1] = fm_mfma_f64(a1, b1, acc[1][1]);
            }
            __syncthreads();
        }
        // the tile's squared distances over the staging buffers (nobody reads those any more); +inf where the pair does not exist
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int li = wi * 32 + 16 * p + kq + 4 * g, lj = wj * 32 + 16 * q + l15;
                    const int i = i0 + li, j = tile * kFmTile + lj;
                    const double v = (nxs[li] + nys[lj]) - 2.0 * acc[p][q][g];
                    const double d2 = v > 0.0 ? v : 0.0;          // +0 for -0 and for a negative rounding residue
                    const bool exists = j < a.m && !(a.exclude_self && j == i);
                    smem[li * kFmDistPitch + lj] = exists ? d2 : inf;
                }
        __syncthreads();
#pragma unroll 4
        for (int e = 0; e < kFmTile / kFmWaves; ++e) {
            const double v = smem[r * kFmDistPitch + c0 + e];
            if (kBall) {
                count += v < rhos[c0 + e] ? 1 : 0;
                nearest = v < nearest ? v : nearest;
            } else {
                keep_smallest(best, v);
            }
        }
        __syncthreads();
    }

    // the four threads of a row, in the order of their columns
    const int64_t slot = (int64_t)sp * a.n + (i0 + tid);          // meaningful where tid < 64
    if (kBall) {
        smem[r * (kFmWaves + 1) + wave] = nearest;
        cnts[r * kFmWaves + wave] = count;
        __syncthreads();
        if (tid < kFmTile && i0 + tid < a.n) {
            int total = 0;
            double lowest = inf;
#pragma unroll
            for (int w = 0; w < kFmWaves; ++w) {
                total += cnts[tid * kFmWaves + w];
                const double v = smem[tid * (kFmWaves + 1) + w];
                lowest = v < lowest ? v : lowest;
            }
            a.cnt[slot] = total;
            a.near[slot] = lowest;
        }
    } else {
#pragma unroll
        for (int t = 0; t < kFmMaxK; ++t) smem[r * kFmMergePitch + wave * kFmMaxK + t] = best[t];
        __syncthreads();
        if (tid < kFmTile && i0 + tid < a.n) {
            double fin[kFmMaxK];
#pragma unroll
            for (int t = 0; t < kFmMaxK; ++t) fin[t] = inf;
            for (int s = 0; s < kFmWaves * kFmMaxK; ++s) keep_smallest(fin, smem[tid * kFmMergePitch + s]);
#pragma unroll
            for (int t = 0; t < kFmMaxK; ++t)
                if (t < a.k) a.lists[slot * a.k + t] = fin[t];
        }
    }
}

// ---- the splits of a row, in the order s = 0, 1, ... -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFmThreads) void knn_finish_kernel(const double* __restrict__ parts, int n, int k, int splits, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kFmThreads + threadIdx.x;
    if (i >= n) return;
    double best[kFmMaxK];
#pragma unroll
    for (int t = 0; t < kFmMaxK; ++t) best[t] = __builtin_inf();
    for (int s = 0; s < splits; ++s)
        for (int t = 0; t < k; ++t) keep_smallest(best, parts[((int64_t)s * n + i) * k + t]);
#pragma unroll
    for (int t = 0; t < kFmMaxK; ++t)
        if (t < k) out[i * k + t] = best[t];
}

__global__ __launch_bounds__(kFmThreads) void ball_finish_kernel(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_near, int n,
                                                                 int splits, int32_t* __restrict__ cnt, double* __restrict__ near) {
    const int64_t i = (int64_t)blockIdx.x * kFmThreads + threadIdx.x;
    if (i >= n) return;
    int total = 0;
    double lowest = __builtin_inf();
    for (int s = 0; s < splits; ++s) {
        total += part_cnt[(int64_t)s * n + i];
        const double v = part_near[(int64_t)s * n + i];
        lowest = v < lowest ? v : lowest;
    }
    cnt[i] = total;
    near[i] = lowest;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static inline int rows_splits(int n, int m, int splits) {
    const int tiles = ceil_div(m, kFmTile), blocks = ceil_div(n, kFmTile);
    if (splits == 0) splits = ceil_div(kFmTargetGroups, blocks);
    return splits < tiles ? (splits < kFmMaxSplits ? splits : kFmMaxSplits) : (tiles < kFmMaxSplits ? tiles : kFmMaxSplits);
}

// k == 0: ball counts
static inline int rows_check(int n, int m, int k, int splits) {
    return n < 1 || m < 1 || n > kFmMaxRows || m > kFmMaxRows || k < 0 || k > kFmMaxK || splits < 0 ? NPCD_ERR_UNSUPPORTED : NPCD_OK;
}

static inline int features_check(int dtype, int D) {
    return D < 1 || D > kFmMaxD || (dtype != NPCD_F32 && dtype != NPCD_F64) ? NPCD_ERR_UNSUPPORTED : NPCD_OK;
}

static inline int64_t rows_workspace_doubles(int n, int m, int k, int splits) {
    const int64_t S = rows_splits(n, m, splits);
    return (int64_t)n + m + (S > 1 ? S * n * (k ? k : 2) : 0);
}

template <class T>
static int launch_norms(const RowsArgs& a, double* nx, double* ny, hipStream_t s) {
    hipLaunchKernelGGL(feature_norms_kernel<T>, dim3((unsigned)ceil_div(a.n, kFmWaves)), dim3(kFmThreads), 0, s, (const T*)a.x, a.ldx, a.n, a.D, nx);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(feature_norms_kernel<T>, dim3((unsigned)ceil_div(a.m, kFmWaves)), dim3(kFmThreads), 0, s, (const T*)a.y, a.ldy, a.m, a.D, ny);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

template <class T, bool kBall>
static int launch_rows(const RowsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((feature_rows_kernel<T, kBall>), dim3((unsigned)(a.row_blocks * a.splits)), dim3(kFmThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_feature_knn_max_k(void) { return kFmMaxK; }

extern "C" int64_t npcd_feature_rows_workspace_bytes(int n, int m, int k, int splits) {
    const int rc = rows_check(n, m, k, splits);
    if (rc != NPCD_OK) return rc;
    return rows_workspace_doubles(n, m, k, splits) * (int64_t)sizeof(double);
}

extern "C" int npcd_feature_knn(const void* x, const void* y, int dtype, int n, int m, int D, int64_t ldx, int64_t ldy, int exclude_self, int k,
                                int splits, double* workspace, double* out, void* stream) {
    int rc = features_check(dtype, D);
    if (rc == NPCD_OK) rc = rows_check(n, m, k, splits);
    if (rc != NPCD_OK) return rc;
    if (k < 1 || (exclude_self != 0 && exclude_self != 1) || (int64_t)m - exclude_self < k) return NPCD_ERR_UNSUPPORTED;
    if (!x || !y || !workspace || !out || ldx < D || ldy < D) return NPCD_ERR_ARG;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int S = rows_splits(n, m, splits);
    double *nx = workspace, *ny = workspace + n, *parts = ny + m;
    RowsArgs a{x, y, ldx, ldy, nx, ny, nullptr, S > 1 ? parts : out, nullptr, nullptr, n, m, D, k, S, ceil_div(m, kFmTile), ceil_div(n, kFmTile),
               exclude_self};
    rc = dtype == NPCD_F32 ? launch_norms<float>(a, nx, ny, s) : launch_norms<double>(a, nx, ny, s);
    if (rc != NPCD_OK) return rc;
    rc = dtype == NPCD_F32 ? launch_rows<float, false>(a, s) : launch_rows<double, false>(a, s);
    if (rc != NPCD_OK) return rc;
    if (S > 1) {
        hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)ceil_div(n, kFmThreads)), dim3(kFmThreads), 0, s, parts, n, k, S, out);
        NPCD_HIP_CHECK(hipGetLastError());
    }
    return NPCD_OK;
}

extern "C" int npcd_feature_ball_counts(const void* x, const void* y, int dtype, int n, int m, int D, int64_t ldx, int64_t ldy, const double* rho_y,
                                        int splits, double* workspace, int32_t* cnt, double* near, void* stream) {
    int rc = features_check(dtype, D);
    if (rc == NPCD_OK) rc = rows_check(n, m, 0, splits);
    if (rc != NPCD_OK) return rc;
    if (!x || !y || !rho_y || !workspace || !cnt || !near || ldx < D || ldy < D) return NPCD_ERR_ARG;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int S = rows_splits(n, m, splits);
    double *nx = workspace, *ny = workspace + n, *part_near = ny + m;
    int32_t* part_cnt = reinterpret_cast<int32_t*>(part_near + (int64_t)S * n);
    RowsArgs a{x, y, ldx, ldy, nx, ny, rho_y, nullptr, S > 1 ? part_cnt : cnt, S > 1 ? part_near : near, n, m, D, 0, S, ceil_div(m, kFmTile),
               ceil_div(n, kFmTile), 0};
    rc = dtype == NPCD_F32 ? launch_norms<float>(a, nx, ny, s) : launch_norms<double>(a, nx, ny, s);
    if (rc != NPCD_OK) return rc;
    rc = dtype == NPCD_F32 ? launch_rows<float, true>(a, s) : launch_rows<double, true>(a, s);
    if (rc != NPCD_OK) return rc;
    if (S > 1) {
        hipLaunchKernelGGL(ball_finish_kernel, dim3((unsigned)ceil_div(n, kFmThreads)), dim3(kFmThreads), 0, s, part_cnt, part_near, n, S, cnt, near);
        NPCD_HIP_CHECK(hipGetLastError());
    }
    return NPCD_OK;
}
