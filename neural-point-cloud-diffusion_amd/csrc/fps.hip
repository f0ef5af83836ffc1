// Farthest point sampling: the operator behind `pytorch3d.ops.sample_farthest_points`, which the reference's dataset
// uses to cut every object's raw surface cloud down to the num_points (512) points of stage 1 (npcd/data/srn.py:179-188).
//
//   cloud i, length L = lengths[i] (P when NULL), K = ks[i] (Kmax when NULL), start s = start[i] (0 when NULL)
//   min_dist[p] = +inf for p < L;  pick_0 = s
//   after pick c:  d = ((x_p - x_c)^2 + (y_p - y_c)^2) + (z_p - z_c)^2   (fp32, as written: cloud_sqdist of clouds.h, no FMA contraction)
//                  min_dist[p] = min(min_dist[p], d)
//   next pick = the p < L with the largest min_dist, the LOWEST index on a tie
//   min(K, L, Kmax) picks; the slots after them hold index -1 and point 0.0
//
// The choice is a max-reduction over the 64-bit key (bits(min_dist) << 32) | (0xFFFFFFFF - p): non-negative floats order as their bit
// patterns, and the complemented index makes the lowest index the largest key among equal distances.  Integer maxima are associative
// and commutative, so the result does not depend on how the reduction is shaped: the same bits on every run.
//
// One workgroup of 1024 threads per cloud, no cooperation between workgroups, no spin-wait: the only loop is the picks, bounded by an
// argument.  A thread owns the points p = j * 1024 + tid.  Two forms of one pick loop:
//   resident   P <= 16 * 1024: coordinates and min_dist of the owned points stay in registers (4 per point)
//   streaming  P <= 100 * 1024: only min_dist stays in registers, the coordinates are read again at every pick with coalesced,
//              point-strided loads (a 100,000-point cloud is 1.2 MB: it stays in the XCD's 4 MiB L2).  Two instantiations: up to
//              32 * 1024 points 32 registers of min_dist leave room for 8 points' loads in flight, above that 100 registers for 4
// A pick: per-thread update and running best (strict > over ascending p keeps the lowest index), DPP max-reduction of the key across
// the wave (wave_max_u64 of wave.h), one key per wave into a double-buffered 16-entry LDS slot, ONE barrier, then every wave reduces
// the 16 keys for itself (nothing is broadcast back).  Buffer (k & 1) is written again at pick k + 2, i.e. after barrier k + 1, which
// no wave passes before every wave has finished reading at pick k.  The winner's coordinates are read from global memory
// (wave-uniform, L2).
// Inputs are assumed finite (not checked).  lengths and start are clamped to [0, P] and [0, L) so that no value of theirs can make
// the kernel read outside the cloud.
#include "clouds.h"

namespace npcd {

constexpr int kFpsThreads = 1024, kFpsWaves = kFpsThreads / kWave;
constexpr int kFpsResident = 16;      // owned points per thread, resident form: 64 registers of state
constexpr int kFpsStreamMid = 32;     // streaming form, clouds up to 32 * 1024 points: room for 8 points' loads in flight
constexpr int kFpsStream = 100;       // streaming form, the largest clouds: 100 registers of min_dist leave room for 4 points' loads

struct FpsArgs {
    const float* points;       // [N, P, 3]
    const int32_t *lengths, *ks, *start;       // [N] each, any may be NULL
    int64_t* idx;              // [N, Kmax]
    float* sel;                // [N, Kmax, 3]
    int P, Kmax;
};

__device__ __forceinline__ uint64_t fps_key(float md, uint32_t p) { return ((uint64_t)__float_as_uint(md) << 32) | (0xFFFFFFFFu - p); }

// a thread owns kOwned points: with their coordinates (STREAM = false), or min_dist only, the coordinates read kFpsChunk points at a
// time at every pick (STREAM = true)
template <int kOwned, int kFpsChunk, bool STREAM>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(FpsArgs a) {
    static_assert(kOwned % kFpsChunk == 0, "the update loop runs whole chunks");
    __shared__ uint64_t slot[2][kFpsWaves];
    const int cloud = blockIdx.x, tid = threadIdx.x, P = a.P, Kmax = a.Kmax;
    const float* __restrict__ pts = a.points + (int64_t)cloud * P * 3;
    int64_t* __restrict__ idx = a.idx + (int64_t)cloud * Kmax;
    float* __restrict__ sel = a.sel + (int64_t)cloud * Kmax * 3;
    const int L = min(max(a.lengths ? a.lengths[cloud] : P, 0), P);
    const int npick = min(min(a.ks ? a.ks[cloud] : Kmax, Kmax), L);      // <= 0: nothing is picked
    // the unused slots
    for (int k = max(npick, 0) + tid; k < Kmax; k += kFpsThreads) {
        idx[k] = -1;
        sel[3 * k] = 0.f;
        sel[3 * k + 1] = 0.f;
        sel[3 * k + 2] = 0.f;
    }
    if (npick <= 0) return;            // the whole workgroup: no barrier is left waiting

    float md[kOwned];
    float px[STREAM ? 1 : kOwned], py[STREAM ? 1 : kOwned], pz[STREAM ? 1 : kOwned];
    const float inf = __uint_as_float(0x7f800000u);
#pragma unroll
    for (int j = 0; j < kOwned; ++j) {
        const int p = j * kFpsThreads + tid;
        md[j] = p < L ? inf : -1.f;           // -1 never wins (strict > from -1) and stays -1 under min with d >= 0
        if constexpr (!STREAM) {
            const bool valid = p < L;
            px[j] = valid ? pts[3 * p] : 0.f;
            py[j] = valid ? pts[3 * p + 1] : 0.f;
            pz[j] = valid ? pts[3 * p + 2] : 0.f;
        }
    }

    int cur = min(max(a.start ? a.start[cloud] : 0, 0), L - 1);
    for (int k = 0;; ++k) {
        cur = __builtin_amdgcn_readfirstlane(cur);
        const float cx = pts[3 * cur], cy = pts[3 * cur + 1], cz = pts[3 * cur + 2];
        if (tid == 0) {
            idx[k] = cur;
            sel[3 * k] = cx;
            sel[3 * k + 1] = cy;
            sel[3 * k + 2] = cz;
        }
        if (k + 1 >= npick) break;
        float best = -1.f;
        uint32_t best_p = 0;
        if constexpr (!STREAM) {
#pragma unroll
            for (int j0 = 0; j0 < kOwned; j0 += kFpsChunk) {
                if (j0 * kFpsThreads < L) {          // workgroup-uniform
#pragma unroll
                    for (int j = j0; j < j0 + kFpsChunk; ++j) {
                        const float d = cloud_sqdist(px[j], py[j], pz[j], cx, cy, cz);
                        md[j] = fminf(md[j], d);
                        if (md[j] > best) {
                            best = md[j];
                            best_p = (uint32_t)(j * kFpsThreads + tid);
                        }
                    }
                }
            }
        } else {
            // the cloud's offset and length pass through an empty asm at every pick: otherwise the compiler keeps one 64-bit address
            // per owned point across the picks, and the 100 registers of min_dist no longer fit
            uint32_t zero = 0;
            int Lk = L;
            asm volatile("" : "+s"(zero), "+s"(Lk));
            const float* base = pts + zero;
#pragma unroll
            for (int j0 = 0; j0 < kOwned; j0 += kFpsChunk) {
                if (j0 * kFpsThreads < Lk) {          // workgroup-uniform
                    // the chunk that holds the cloud's end re-reads the last point for the points past it (their md stays -1): no lane
                    // is masked and the loads of a chunk are in flight together
                    const bool whole = (j0 + kFpsChunk) * kFpsThreads <= Lk;
                    float x[kFpsChunk], y[kFpsChunk], z[kFpsChunk];
#pragma unroll
                    for (int q = 0; q < kFpsChunk; ++q) {
                        const int p = (j0 + q) * kFpsThreads + tid;
                        const float* pp = base + 3u * (uint32_t)(whole ? p : min(p, Lk - 1));          // 0 <= index < L
                        x[q] = pp[0];
                        y[q] = pp[1];
                        z[q] = pp[2];
                    }
#pragma unroll
                    for (int q = 0; q < kFpsChunk; ++q) {
                        const int j = j0 + q;
                        const float d = cloud_sqdist(x[q], y[q], z[q], cx, cy, cz);
                        md[j] = fminf(md[j], d);
                        if (md[j] > best) {
                            best = md[j];
                            best_p = (uint32_t)(j * kFpsThreads + tid);
                        }
                    }
                }
            }
        }
        const uint64_t wkey = wave_max_u64(best < 0.f ? 0ull : fps_key(best, best_p));
        int mine = tid;          // derived again at every pick (empty asm): the streaming form has no registers to keep LDS addresses in
        asm volatile("" : "+v"(mine));
        if ((mine & (kWave - 1)) == 0) slot[k & 1][mine / kWave] = wkey;
        __syncthreads();
        const uint64_t all = read_lane(row_max_u64(slot[k & 1][mine & (kFpsWaves - 1)]), 15);
        // a valid point always exists here (L >= 1), so the key is never 0; the clamp keeps even a NaN-ridden cloud inside its rows
        cur = (int)min(0xFFFFFFFFu - (uint32_t)all, (uint32_t)(L - 1));
    }
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_fps_resident_points(void) { return kFpsResident * kFpsThreads; }
extern "C" int npcd_fps_max_points(void) { return kFpsStream * kFpsThreads; }

extern "C" int npcd_fps(const float* points, const int32_t* lengths, const int32_t* ks, const int32_t* start, int64_t* idx_out, float* pts_out,
                        int N, int P, int Kmax, void* stream) {
    if (N <= 0 || P <= 0 || Kmax <= 0 || P > kFpsStream * kFpsThreads) return NPCD_ERR_UNSUPPORTED;
    if (!points || !idx_out || !pts_out) return NPCD_ERR_ARG;
    const FpsArgs a{points, lengths, ks, start, idx_out, pts_out, P, Kmax};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P <= kFpsResident * kFpsThreads)
        hipLaunchKernelGGL((fps_kernel<kFpsResident, 4, false>), dim3(N), dim3(kFpsThreads), 0, st, a);
    else if (P <= kFpsStreamMid * kFpsThreads)
        hipLaunchKernelGGL((fps_kernel<kFpsStreamMid, 8, true>), dim3(N), dim3(kFpsThreads), 0, st, a);
    else
        hipLaunchKernelGGL((fps_kernel<kFpsStream, 4, true>), dim3(N), dim3(kFpsThreads), 0, st, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
