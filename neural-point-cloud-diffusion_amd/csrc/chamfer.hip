// All-pairs directed Chamfer matrix: the distance under the shape metrics MMD-CD / COV-CD / 1-NNA-CD of npcd/eval/shapes.py.
//
//   X [M, P, 3], Y [N, Q, 3] fp32;  Lx_i = clamp(x_len[i], 1, P) (P when NULL), Ly_j = clamp(y_len[j], 1, Q) (Q when NULL)
//   out[i, j] = ( sum_{p < Lx_i}  min_{q < Ly_j}  d(x_ip, y_jq) ) / Lx_i
//   d(a, b)   = ((dx dx + dy dy) + dz dz),  dx = a.x - b.x ...   (cloud_sqdist of clouds.h: fp32, as written, no FMA contraction)
//
// min is exact, so every per-point minimum is the bits of a numpy fp32 evaluation of d; only the sum over p and the division round.
// The sum has one fixed order (the lane's points in ascending p, wave_sum_tree of wave.h over the lanes, the four waves in ascending
// order) and there is no atomic: the same bits on every run.  The norm-expansion form |a|^2 + |b|^2 - 2 a.b is not used anywhere: it
// cancels exactly at the nearest pairs, the only distances that are kept.
//
// One workgroup of 256 lanes owns G X clouds in registers, PPL points of each per lane (point p = k * 256 + tid), with one running
// minimum per owned point: <PPL, G> = <1, 8> up to 256 points, <2, 4> up to 512, <4, 2> up to 1,024, <8, 1> up to 2,048 (8 owned
// points each) and <16, 1> up to 4,096.  It walks a chunk of Y clouds; each is staged through LDS in tiles of kChamferTile rows, a
// straight copy of its packed 12-byte rows, while the tile before is consumed (two buffers, one barrier per tile).  The loop reads
// four rows as three 16-byte LDS words -- every lane the same address, a broadcast -- and spends 9 lane-operations per point pair
// (3 subtractions, 3 multiplications, 2 additions, 1 minimum), so 72 (144) of them per row read.  A tile's rows are padded to a
// multiple of four with copies of the cloud's last valid row, which cannot change a minimum.  After a Y cloud's last tile the minima
// are summed and out[i, j] is stored once; nothing else is written.
// No read leaves the arrays whatever the lengths hold: an X row at or after Lx_i is not loaded (the lane keeps zeros and its minima
// are left out of the sum), Y rows are addressed through min(row, Ly_j - 1).  X and Y are only read and may be the same pointer.
#include "clouds.h"

namespace npcd {

constexpr int kChamferThreads = kCloudPairThreads, kChamferWaves = kChamferThreads / kWave;
constexpr int kChamferTile = 512;                              // Y rows per LDS tile
constexpr int kChamferTileWords = kChamferTile * 3;            // fp32 words of a tile: 6 KiB
constexpr int kChamferStage = kChamferTileWords / kChamferThreads;          // words a lane stages per tile
constexpr int kChamferMaxPoints = 16 * kChamferThreads;        // the largest instantiation
static_assert(kChamferTileWords % kChamferThreads == 0 && kChamferTile % 4 == 0, "whole staging rounds, whole groups of four rows");

// tile `t` of a Y cloud of `L` valid rows at `yj`: the words this lane stages.  Word w of the tile is coordinate w % 3 of tile row
// w / 3; rows past the cloud's end, up to the next multiple of four, repeat row L - 1; words past that are not used and not read.
__device__ __forceinline__ void chamfer_fetch(const float* __restrict__ yj, int L, int t, int tid, float (&pre)[kChamferStage]) {
    const int base = t * kChamferTile;
    const int rows4 = (min(kChamferTile, L - base) + 3) & ~3;
#pragma unroll
    for (int k = 0; k < kChamferStage; ++k) {
        const int w = k * kChamferThreads + tid, r = w / 3, c = w - 3 * r;
        pre[k] = r < rows4 ? yj[3 * (int64_t)min(base + r, L - 1) + c] : 0.f;          // 0 <= row < L <= Q
    }
}

template <int PPL, int G>
__global__ __launch_bounds__(kChamferThreads) void chamfer_kernel(CloudPairArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[2][kChamferTileWords];
    __shared__ float part[2][G][kChamferWaves];
    const int tid = threadIdx.x;
    const int group = blockIdx.x / a.nchunks, chunk = blockIdx.x - group * a.nchunks;
    const int j0 = chunk * a.chunk, j1 = min(j0 + a.chunk, a.N);          // j0 < N by the grid's size
    const int P = a.P, Q = a.Q;

    // the owned X points
    float px[G][PPL], py[G][PPL], pz[G][PPL], mn[G][PPL];
    bool valid[G][PPL];
    const float inf = __uint_as_float(0x7f800000u);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int i = group * G + g;
        const int Lx = i < a.M ? cloud_len(a.x_len, i, P) : 0;
        const float* __restrict__ xi = a.x + (int64_t)min(i, a.M - 1) * P * 3;
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
            const int p = k * kChamferThreads + tid;
            valid[g][k] = p < Lx;
            px[g][k] = valid[g][k] ? xi[3 * p] : 0.f;
            py[g][k] = valid[g][k] ? xi[3 * p + 1] : 0.f;
            pz[g][k] = valid[g][k] ? xi[3 * p + 2] : 0.f;
            mn[g][k] = inf;
        }
    }

    // the first tile
    int j = j0, t = 0;
    int Ly = cloud_len(a.y_len, j, Q);
    float pre[kChamferStage];
    chamfer_fetch(a.y + (int64_t)j * Q * 3, Ly, 0, tid, pre);
#pragma unroll
    for (int k = 0; k < kChamferStage; ++k) tile[0][k * kChamferThreads + tid] = pre[k];
    __syncthreads();

    for (int step = 0;; ++step) {
        const int buf = step & 1;
        const int ntiles = (Ly + kChamferTile - 1) / kChamferTile;
        const bool last_tile = t + 1 == ntiles;
        // the step after this one: the cloud's next tile, or the next cloud's first
        const int nj = last_tile ? j + 1 : j, nt = last_tile ? 0 : t + 1;
        const bool more = nj < j1;
        const int nLy = more ? (last_tile ? cloud_len(a.y_len, nj, Q) : Ly) : 1;
        if (more) chamfer_fetch(a.y + (int64_t)nj * Q * 3, nLy, nt, tid, pre);

        const int groups4 = (min(kChamferTile, Ly - t * kChamferTile) + 3) >> 2;
        const f32x4* __restrict__ rows = reinterpret_cast<const f32x4*>(tile[buf]);
#pragma unroll 2
        for (int q4 = 0; q4 < groups4; ++q4) {
            const f32x4 u = rows[3 * q4], v = rows[3 * q4 + 1], w = rows[3 * q4 + 2];
#pragma unroll
            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int k = 0; k < PPL; ++k) {
                    const float d0 = cloud_sqdist(px[g][k], py[g][k], pz[g][k], u[0], u[1], u[2]);
                    const float d1 = cloud_sqdist(px[g][k], py[g][k], pz[g][k], u[3], v[0], v[1]);
                    const float d2 = cloud_sqdist(px[g][k], py[g][k], pz[g][k], v[2], v[3], w[0]);
                    const float d3 = cloud_sqdist(px[g][k], py[g][k], pz[g][k], w[1], w[2], w[3]);
                    mn[g][k] = fminf(fminf(fminf(fminf(mn[g][k], d0), d1), d2), d3);
                }
            }
        }

        if (last_tile) {
            // the lane's valid minima in ascending p, then the wave; one partial per wave and X cloud
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < PPL; ++k) {
                    s += valid[g][k] ? mn[g][k] : 0.f;
                    mn[g][k] = inf;
                }
                s = wave_sum_tree(s);
                if ((tid & (kWave - 1)) == 0) part[j & 1][g][tid / kWave] = s;
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < kChamferStage; ++k) tile[buf ^ 1][k * kChamferThreads + tid] = pre[k];
        }
        // one barrier per step: the next tile is complete, this tile is free to be overwritten at the next step, and the partials
        // of cloud j are visible.  part[j & 1] is written again for cloud j + 2, behind the barrier of cloud j + 1's last step, which
        // no wave passes before the lanes below have read.
        __syncthreads();
        if (last_tile && tid < G) {
            const int i = group * G + tid;
            if (i < a.M) {
                float s = part[j & 1][tid][0];
#pragma unroll
                for (int wv = 1; wv < kChamferWaves; ++wv) s += part[j & 1][tid][wv];
                a.out[(int64_t)i * a.N + j] = s / (float)cloud_len(a.x_len, i, P);
            }
        }
        if (!more) break;
        j = nj;
        t = nt;
        Ly = nLy;
    }
}

template <int PPL, int G>
static void chamfer_launch(CloudPairArgs a, hipStream_t st) {
    const int64_t groups = (a.M + G - 1) / G;
    cloud_pair_chunks(groups, a.N, &a.chunk, &a.nchunks);
    hipLaunchKernelGGL((chamfer_kernel<PPL, G>), dim3((unsigned)(groups * a.nchunks)), dim3(kChamferThreads), 0, st, a);
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_chamfer_max_points(void) { return kChamferMaxPoints; }

extern "C" int npcd_chamfer_directed(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, float* out, int M, int P,
                                     int N, int Q, void* stream) {
    const int rc = cloud_pair_check(x, y, out, M, P, N, Q, kChamferMaxPoints);
    if (rc != NPCD_OK) return rc;
    const CloudPairArgs a{x, y, x_len, y_len, out, M, P, N, Q, 0, 0};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P <= 1 * kChamferThreads)
        chamfer_launch<1, 8>(a, st);
    else if (P <= 2 * kChamferThreads)
        chamfer_launch<2, 4>(a, st);
    else if (P <= 4 * kChamferThreads)
        chamfer_launch<4, 2>(a, st);
    else if (P <= 8 * kChamferThreads)
        chamfer_launch<8, 1>(a, st);
    else
        chamfer_launch<16, 1>(a, st);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
