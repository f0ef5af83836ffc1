// All-pairs directed approximate earth mover's distance: the second distance under the shape metrics of
// npcd/eval/shapes.py (MMD-EMD / COV-EMD / 1-NNA-EMD), the approximate matching of Fan et al. with its fixed trip count.
//
//   X [M, P, 3], Y [N, Q, 3] fp32;  Lx = clamp(x_len[i], 1, P) (P when NULL), Ly = clamp(y_len[j], 1, Q) (Q when NULL), T = max(Lx, Ly)
//   d(l, k) = ((dx dx + dy dy) + dz dz) on direct differences (cloud_sqdist of clouds.h: fp32, as written, no FMA contraction)
//   remainL[l] = T / Lx, remainR[k] = T / Ly, cost = 0; for level in -4^7, -4^6 ... -4^0, -4^-1, 0:
//     e(l, k)   = exp(level d(l, k))
//     ratioL[l] = remainL[l] / (1e-9 + sum_k e(l, k) remainR[k])                          pass A, rows
//     sumr      = remainR[k] sum_l e(l, k) ratioL[l]                                      pass B, columns
//     ratioR[k] = min(remainR[k] / (sumr + 1e-9), 1) remainR[k];  remainR[k] = max(0, remainR[k] - sumr)
//     w(l, k)   = e(l, k) ratioL[l] ratioR[k]                                             pass C, rows
//     cost     += sum_lk w(l, k) sqrt(d(l, k));  remainL[l] = max(0, remainL[l] - sum_k w(l, k))
//   out[i, j] = cost / T
//
// One workgroup of 256 lanes owns one X cloud and walks a chunk of Y clouds, one pair at a time.  For the pair, LDS holds both clouds
// as packed 12-byte rows, ratioL (one float per X row) and remainR / ratioR (one float per Y row) -- dynamic LDS, 256 (16 PPL + 20 QPL)
// bytes, sized by the instantiation: 9 KiB at 256 points a side, 18 KiB at 512, 72 KiB at 2,048 --; remainL lives in the registers of
// the row's owner.  Lane tid owns rows tid + 256 r, r < PPL, in passes A and C and columns tid + 256 c, c < QPL, in pass B; it walks
// the other cloud four rows at a time through three 16-byte coordinate reads and one 16-byte weight read, every lane the same
// address (a broadcast).  PPL and QPL are template parameters chosen from P and Q (1, 2, 4, 8): sixteen instantiations, no run-time
// form of the inner loops.  Owned groups that lie wholly at or after the cloud's length are skipped by a workgroup-uniform test.
//
// Sums: a row sum or a column sum is ONE accumulator in the owner lane, the walked points in ascending index, e times the weight
// fused into the addition (one rounding); it never crosses lanes.  The row's factor ratioL is applied once to the finished row sums
// of pass C.  cost is one accumulator per lane over the levels and the lane's rows in ascending order; it crosses lanes once per pair:
// a fixed tree over the wave (wave_sum_tree of wave.h), then the four waves in ascending order.  No atomics: the same bits on every run.
// exp is v_exp_f32 on the level pre-multiplied by log2(e), sqrt is v_sqrt_f32.
//
// Tails: both clouds are staged whole, every row of the instantiation, through min(row, L - 1): rows at or after the length are
// copies of the last valid row and carry weight 0 for ever (remainL = ratioL = 0, remainR = ratioR = 0), so walking them to the next
// multiple of four adds exact zeros.  No read leaves the arrays whatever the lengths hold.  X and Y are only read and may be the same
// pointer.
#include "clouds.h"

namespace npcd {

constexpr int kEmdThreads = kCloudPairThreads, kEmdWaves = kEmdThreads / kWave;
constexpr int kEmdMaxPoints = 8 * kEmdThreads;              // the largest instantiation
constexpr int kEmdLevels = 10;

// dynamic LDS of emd_kernel<PPL, QPL>: both clouds as 12-byte rows, ratioL per X row, remainR and ratioR per Y row
constexpr size_t emd_lds_bytes(int ppl, int qpl) { return (size_t)kEmdThreads * (16 * ppl + 20 * qpl); }
static_assert(emd_lds_bytes(8, 8) + 64 <= 160 * 1024, "the largest pair does not fit the LDS of a compute unit");

// a cloud of L valid rows into its LDS image of ROWS rows: row r is row min(r, L - 1) of the cloud
template <int ROWS>
__device__ __forceinline__ void emd_stage(float* __restrict__ dst, const float* __restrict__ src, int L, int tid) {
#pragma unroll 3          // a few loads in flight; unrolled whole, the 24 addresses of the largest image cost 70 registers
    for (int k = 0; k < ROWS * 3 / kEmdThreads; ++k) {
        const int w = k * kEmdThreads + tid, r = w / 3, c = w - 3 * r;
        dst[w] = src[3 * (int64_t)min(r, L - 1) + c];          // 0 <= row < L
    }
}

// OWN points of this lane (point o * 256 + tid of `mine`) against the first `walked4` groups of four rows of `other`, weights wt:
// s = sum_k exp2(lvl d) wt[k], one accumulator, ascending k, and with COST also c = sum_k (exp2(lvl d) wt[k]) sqrt(d); then
// done(o, s, c) for every owned point, skipped groups included (s = c = 0).  At most four owned points are walked at a time: eight
// take two walks, each with its own `done`, so that no more than four sets of sums and of the divisions behind them are ever live.
template <int OWN, bool COST, typename Done>
__device__ __forceinline__ void emd_walk(const float* __restrict__ mine, const float* __restrict__ other, const float* __restrict__ wt,
                                         int groups, int walked4, float lvl, int tid, Done done) {
    constexpr int BLK = OWN < 4 ? OWN : 4;
    const f32x4* __restrict__ rows = reinterpret_cast<const f32x4*>(other);
    const f32x4* __restrict__ wts = reinterpret_cast<const f32x4*>(wt);
#pragma unroll
    for (int o0 = 0; o0 < OWN; o0 += BLK) {
        float px[BLK], py[BLK], pz[BLK], s[BLK], c[BLK];
#pragma unroll
        for (int o = 0; o < BLK; ++o) {
            const int p = (o0 + o) * kEmdThreads + tid;
            px[o] = mine[3 * p], py[o] = mine[3 * p + 1], pz[o] = mine[3 * p + 2];
            s[o] = 0.f;
            c[o] = 0.f;
        }
        if (o0 < groups) {          // workgroup-uniform, as is every test against `groups`
#pragma unroll 1
            for (int q4 = 0; q4 < walked4; ++q4) {
                const f32x4 u = rows[3 * q4], v = rows[3 * q4 + 1], w = rows[3 * q4 + 2], g = wts[q4];
#pragma unroll
                for (int o = 0; o < BLK; ++o) {
                    if (o0 + o < groups) {
                        const float d0 = cloud_sqdist(px[o], py[o], pz[o], u[0], u[1], u[2]);
                        const float d1 = cloud_sqdist(px[o], py[o], pz[o], u[3], v[0], v[1]);
                        const float d2 = cloud_sqdist(px[o], py[o], pz[o], v[2], v[3], w[0]);
                        const float d3 = cloud_sqdist(px[o], py[o], pz[o], w[1], w[2], w[3]);
                        const float e0 = __builtin_amdgcn_exp2f(lvl * d0), e1 = __builtin_amdgcn_exp2f(lvl * d1);
                        const float e2 = __builtin_amdgcn_exp2f(lvl * d2), e3 = __builtin_amdgcn_exp2f(lvl * d3);
                        if (COST) {
                            const float t0 = e0 * g[0], t1 = e1 * g[1], t2 = e2 * g[2], t3 = e3 * g[3];
                            s[o] = (((s[o] + t0) + t1) + t2) + t3;
                            c[o] = __builtin_fmaf(t0, __builtin_amdgcn_sqrtf(d0), c[o]);
                            c[o] = __builtin_fmaf(t1, __builtin_amdgcn_sqrtf(d1), c[o]);
                            c[o] = __builtin_fmaf(t2, __builtin_amdgcn_sqrtf(d2), c[o]);
                            c[o] = __builtin_fmaf(t3, __builtin_amdgcn_sqrtf(d3), c[o]);
                        } else {
                            s[o] = __builtin_fmaf(e0, g[0], s[o]);
                            s[o] = __builtin_fmaf(e1, g[1], s[o]);
                            s[o] = __builtin_fmaf(e2, g[2], s[o]);
                            s[o] = __builtin_fmaf(e3, g[3], s[o]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < BLK; ++o) done(o0 + o, s[o], c[o]);
    }
}

template <int PPL, int QPL>
__global__ __launch_bounds__(kEmdThreads) void emd_kernel(CloudPairArgs a) {
    constexpr int XR = PPL * kEmdThreads, YR = QPL * kEmdThreads;
    // the pair's images, emd_lds_bytes(PPL, QPL) of dynamic LDS; every part is a multiple of 1 KiB long
    extern __shared__ __attribute__((aligned(16))) float emd_lds[];
    float* const xs = emd_lds;                  // [XR, 3]
    float* const ys = xs + XR * 3;              // [YR, 3]
    float* const ratl = ys + YR * 3;            // [XR]
    float* const remr = ratl + XR;              // [YR]
    float* const ratr = remr + YR;              // [YR]
    __shared__ float part[kEmdWaves];
    const int tid = threadIdx.x;
    const int i = blockIdx.x / a.nchunks, chunk = blockIdx.x - i * a.nchunks;          // i < M by the grid's size
    const int j0 = chunk * a.chunk, j1 = min(j0 + a.chunk, a.N);                       // j0 < N by the grid's size
    const int Lx = cloud_len(a.x_len, i, a.P);
    const int xgroups = (Lx + kEmdThreads - 1) / kEmdThreads, x4 = (Lx + 3) >> 2;
    emd_stage<XR>(xs, a.x + (int64_t)i * a.P * 3, Lx, tid);

    for (int j = j0; j < j1; ++j) {
        const int Ly = cloud_len(a.y_len, j, a.Q);
        const int ygroups = (Ly + kEmdThreads - 1) / kEmdThreads, y4 = (Ly + 3) >> 2;
        const float T = (float)max(Lx, Ly);
        // behind the barrier at the end of the pair before: nobody reads ys, remr or ratr any more
        emd_stage<YR>(ys, a.y + (int64_t)j * a.Q * 3, Ly, tid);
        const float massR = T / (float)Ly;
#pragma unroll
        for (int c = 0; c < QPL; ++c) {
            const int k = c * kEmdThreads + tid;
            remr[k] = k < Ly ? massR : 0.f;
            ratr[k] = 0.f;
        }
        float reml[PPL], cost = 0.f;
        const float massL = T / (float)Lx;
#pragma unroll
        for (int r = 0; r < PPL; ++r) reml[r] = r * kEmdThreads + tid < Lx ? massL : 0.f;
        __syncthreads();

        float lvl = -16384.f * kLog2e;
#pragma unroll 1
        for (int level = 0; level < kEmdLevels; ++level, lvl = level == kEmdLevels - 1 ? 0.f : lvl * 0.25f) {
            // pass A
            emd_walk<PPL, false>(xs, ys, remr, xgroups, y4, lvl, tid, [&](int r, float s, float) {
                ratl[r * kEmdThreads + tid] = reml[r] / (1e-9f + s);
            });
            __syncthreads();
            // pass B: the column owner alone reads and writes remr[k] and writes ratr[k]
            emd_walk<QPL, false>(ys, xs, ratl, ygroups, x4, lvl, tid, [&](int c, float s, float) {
                const int k = c * kEmdThreads + tid;
                const float rem = remr[k];
                const float sumr = rem * s;
                ratr[k] = fminf(rem / (sumr + 1e-9f), 1.f) * rem;
                remr[k] = fmaxf(0.f, rem - sumr);
            });
            __syncthreads();
            // pass C: the row's factor ratioL, its owner's own word of ratl, once on the finished sums
            emd_walk<PPL, true>(xs, ys, ratr, xgroups, y4, lvl, tid, [&](int r, float s, float c) {
                const float ratio = ratl[r * kEmdThreads + tid];
                cost += ratio * c;
                reml[r] = fmaxf(0.f, reml[r] - ratio * s);
            });
            // no barrier here: the next pass A reads ys and remr, which nobody writes before the barrier after it, and writes ratl,
            // which was last read in pass B, behind the barrier above
        }

        cost = wave_sum_tree(cost);
        if ((tid & (kWave - 1)) == 0) part[tid / kWave] = cost;
        __syncthreads();          // the partials are visible; every lane is done with this pair's ys, remr and ratr
        if (tid == 0) {
            float s = part[0];
#pragma unroll
            for (int wv = 1; wv < kEmdWaves; ++wv) s += part[wv];
            a.out[(int64_t)i * a.N + j] = s / T;
        }
        // part is written again only behind the 21 barriers of the next pair, which lane 0 passes after this read
    }
}

template <int PPL, int QPL>
static int emd_launch(CloudPairArgs a, hipStream_t st) {
    static DynLds attr;
    const size_t lds = emd_lds_bytes(PPL, QPL);
    NPCD_HIP_CHECK(attr.ensure(reinterpret_cast<const void*>(emd_kernel<PPL, QPL>), lds));
    cloud_pair_chunks(a.M, a.N, &a.chunk, &a.nchunks);
    hipLaunchKernelGGL((emd_kernel<PPL, QPL>), dim3((unsigned)((int64_t)a.M * a.nchunks)), dim3(kEmdThreads), lds, st, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

template <int PPL>
static int emd_launch_q(const CloudPairArgs& a, hipStream_t st) {
    if (a.Q <= 1 * kEmdThreads) return emd_launch<PPL, 1>(a, st);
    if (a.Q <= 2 * kEmdThreads) return emd_launch<PPL, 2>(a, st);
    if (a.Q <= 4 * kEmdThreads) return emd_launch<PPL, 4>(a, st);
    return emd_launch<PPL, 8>(a, st);
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_emd_max_points(void) { return kEmdMaxPoints; }

extern "C" int npcd_emd_directed(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, float* out, int M, int P, int N,
                                 int Q, void* stream) {
    const int rc = cloud_pair_check(x, y, out, M, P, N, Q, kEmdMaxPoints);
    if (rc != NPCD_OK) return rc;
    const CloudPairArgs a{x, y, x_len, y_len, out, M, P, N, Q, 0, 0};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P <= 1 * kEmdThreads) return emd_launch_q<1>(a, st);
    if (P <= 2 * kEmdThreads) return emd_launch_q<2>(a, st);
    if (P <= 4 * kEmdThreads) return emd_launch_q<4>(a, st);
    return emd_launch_q<8>(a, st);
}
