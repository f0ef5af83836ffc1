// Stage-1 regularisers: the inverse-distance weighted L1 variation of the point features over each point's neighbour
// list (neural_point_cloud_tv_loss.py:29-83) and the KL term of the variational feature embedding
// (neural_point_cloud_kl_loss.py:29-44), forward and backward, as one kernel each way.  They replace the ~25 torch operators of
// npcd/losses (masked_scatter_, three boolean-mask gathers, two norms, an index_add_) and autograd's chain behind them; every
// boolean-mask index there is a nonzero, i.e. a host wait.  Nothing here waits on the host and nothing depends on a count.
//
//   tv_i = weight_tv * sum_{j in list(i)} w_ij * sum_f |feat_j - feat_i|,   w_ij = 1 / (|p_j - p_i|_2 + 1e-5)     (list order)
//   kl_i = weight_kl * (-0.5) * sum_f (1 + lv - m^2 - exp(lv))
//   totals = means over B N, from per-cloud partial sums added in ascending cloud order by a one-wave tail launch
//
// LIST RULE.  list(i) is row i of nb: int32 GLOBAL indices b N + j, padded with -1, given with a row stride so that slot 0 of the
// dense query result [B, N, M, k] is read in place.  An entry is SKIPPED when it is negative, when it is the point itself, or when it
// lies outside its own cloud [b N, (b + 1) N).  Skipping the point itself is the torch path's "drop self if there is another
// neighbour; a lost point keeps itself": a self pair adds exactly 0 to value and gradient (|0| = 0, sign(0) = 0).  Entries of another
// cloud never come out of the query; treating them as padding keeps a hand-made or stale list from reading out of bounds.
//
// One workgroup of 1024 threads per cloud, 32 lanes per point (a lane owns the features f = lane + 32 t, t < 4: F <= 128), the cloud's
// coordinates in LDS as 16-byte points.  The backward's neighbour part -- sum over every i' whose list names i -- is a GATHER over a
// reverse table built in LDS: count (integer LDS atomics), exclusive prefix, fill (integer atomics again: arrival order), then every
// segment is sorted by i', so the float sums run in ascending i' whatever the arrival order was.  No float atomic, global or LDS:
// the same bits from run to run.  The lists are streamed from global memory (three coalesced passes in the backward); LDS holds what is
// gathered at random -- coordinates and the reverse table: 64 KiB + 16 KiB offsets + 64 KiB of 16-bit owners at the limits below.
// Coordinates receive no gradient (the reference detaches them).
//
// Supported: fp32, 1 <= N <= 4096, k N <= 32768, 1 <= F <= 128.  Bound: launch latency (8 x 512 x 8 x 32 differences are 4 MFLOP and
// 0.6 MB); compiled without FMA contraction so that the expressions are evaluated as written.
#include "common.h"

namespace npcd {

constexpr int kRegThreads = 1024, kRegLanes = 32, kRegMaxN = 4096, kRegMaxPairs = 32768, kRegMaxF = 128, kRegChunks = kRegMaxF / kRegLanes;
constexpr int kRegWaves = kRegThreads / kWave;
constexpr size_t kCuLds = 160 * 1024;
constexpr size_t reg_fwd_lds(int N) { return (size_t)N * 16 + 2 * kRegWaves * sizeof(float); }
constexpr size_t reg_bwd_lds(int N, int k) {
    return (size_t)N * 16 + (((size_t)N * 4 + 15) & ~(size_t)15) + (((size_t)N * k * 2 + 15) & ~(size_t)15) + kRegWaves * sizeof(int);
}
static_assert(reg_fwd_lds(kRegMaxN) <= kCuLds, "forward LDS exceeds a CU");
static_assert(reg_bwd_lds(kRegMaxN, kRegMaxPairs / kRegMaxN) <= kCuLds, "backward LDS exceeds a CU");
static_assert(kRegMaxN <= 65535, "reverse-table owners are 16-bit");

struct RegArgs {
    const float* coords;       // [B, N, 3]
    const int32_t* nb;         // row i of cloud b at nb[(b N + i) nb_ld], k entries; NULL: no TV term
    int64_t nb_ld;
    const float* feats;        // row stride feats_ld
    int64_t feats_ld;
    const float *mean, *log_var;   // row stride kl_ld; NULL: no KL term
    int64_t kl_ld;
    int N, k, F;
    float weight_tv, weight_kl;
};

// local index of a list entry inside cloud b, or -1 when the entry is skipped (LIST RULE)
__device__ __forceinline__ int reg_local(int32_t e, int b, int N, int self) {
    const int64_t jl = (int64_t)e - (int64_t)b * N;
    return (e < 0 || jl < 0 || jl >= N || jl == self) ? -1 : (int)jl;
}

__device__ __forceinline__ float reg_inv_dist(const float4 a, const float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return 1.f / (sqrtf((dx * dx + dy * dy) + dz * dz) + 1e-5f);
}

__device__ __forceinline__ void reg_load_cloud(const float* __restrict__ coords, int b, int N, float4* pts) {
    for (int i = threadIdx.x; i < N; i += kRegThreads) {
        const float* p = coords + ((int64_t)b * N + i) * 3;
        pts[i] = make_float4(p[0], p[1], p[2], 0.f);
    }
}

// sum over the 32 lanes of a point; every lane gets the same bits (a + b == b + a)
__device__ __forceinline__ float reg_point_sum(float v) {
#pragma unroll
    for (int m = 1; m < kRegLanes; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(kRegThreads) void stage1_reg_fwd_kernel(RegArgs a, float* __restrict__ tv_pw, float* __restrict__ kl_pw,
                                                                     float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* pts = reinterpret_cast<float4*>(smem);
    float* red = reinterpret_cast<float*>(smem + (size_t)a.N * 16);      // [2][waves]
    const int b = blockIdx.x, N = a.N, F = a.F;
    const int lane = threadIdx.x & (kRegLanes - 1), sub = threadIdx.x / kRegLanes;
    constexpr int kSubs = kRegThreads / kRegLanes;
    if (a.nb) reg_load_cloud(a.coords, b, N, pts);
    __syncthreads();
    float sum_tv = 0.f, sum_kl = 0.f;             // lane 0 of each point group: its points in ascending order
    for (int base = 0; base < N; base += kSubs) {
        const bool active = base + sub < N;
        const int i = active ? base + sub : 0;
        const int64_t row = (int64_t)b * N + i;
        if (a.nb) {
            const float4 pi = pts[i];
            const float* fi = a.feats + row * a.feats_ld;
            float acc = 0.f;
            for (int s = 0; s < a.k; ++s) {
                const int jl = reg_local(a.nb[row * a.nb_ld + s], b, N, i);
                const int j = jl < 0 ? i : jl;
                const float* fj = a.feats + ((int64_t)b * N + j) * a.feats_ld;
                float d = 0.f;
#pragma unroll
                for (int t = 0; t < kRegChunks; ++t) {
                    const int f = lane + kRegLanes * t;
                    if (f < F) d += fabsf(fj[f] - fi[f]);
                }
                d = reg_point_sum(d);
                if (jl >= 0) acc += reg_inv_dist(pts[j], pi) * d;
            }
            const float tv = a.weight_tv * acc;
            if (active && lane == 0) {
                tv_pw[row] = tv;
                sum_tv += tv;
            }
        }
        if (a.mean) {
            const float *m = a.mean + row * a.kl_ld, *lv = a.log_var + row * a.kl_ld;
            float d = 0.f;
#pragma unroll
            for (int t = 0; t < kRegChunks; ++t) {
                const int f = lane + kRegLanes * t;
                if (f < F) d += ((1.f + lv[f]) - m[f] * m[f]) - expf(lv[f]);
            }
            d = reg_point_sum(d);
            const float kl = (-0.5f * d) * a.weight_kl;
            if (active && lane == 0) {
                kl_pw[row] = kl;
                sum_kl += kl;
            }
        }
    }
    // the cloud's partial sums: lanes of a wave, then the waves in ascending order
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        sum_tv += __shfl_xor(sum_tv, m, 64);
        sum_kl += __shfl_xor(sum_kl, m, 64);
    }
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red[wave] = sum_tv;
        red[kRegWaves + wave] = sum_kl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f, q = 0.f;
        for (int w = 0; w < kRegWaves; ++w) {
            t += red[w];
            q += red[kRegWaves + w];
        }
        part[2 * b] = t;
        part[2 * b + 1] = q;
    }
}

// fixed-order second stage: the clouds' partial sums in ascending cloud order -> the two means
__global__ __launch_bounds__(kWave) void stage1_reg_totals_kernel(const float* __restrict__ part, int B, float count, float* __restrict__ tv_total,
                                                                  float* __restrict__ kl_total) {
    if (threadIdx.x != 0) return;
    float t = 0.f, q = 0.f;
    for (int b = 0; b < B; ++b) {
        t += part[2 * b];
        q += part[2 * b + 1];
    }
    if (tv_total) *tv_total = t / count;
    if (kl_total) *kl_total = q / count;
}

struct RegGrads {
    const float *tv_total, *tv_pw, *kl_total, *kl_pw;       // upstream gradients: of the mean (one float) and per point [B, N]; any may be NULL
    float *dfeats, *dmean, *dlog_var;                       // [B, N, F] contiguous
};

// the per-point upstream gradient: mean's gradient / (B N) + the pointwise output's gradient
__device__ __forceinline__ float reg_upstream(const float* total, const float* pw, int64_t row, float count) {
    return (total ? *total / count : 0.f) + (pw ? pw[row] : 0.f);
}

__global__ __launch_bounds__(kRegThreads) void stage1_reg_bwd_kernel(RegArgs a, RegGrads g, float count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, N = a.N, F = a.F, k = a.k;
    float4* pts = reinterpret_cast<float4*>(smem);
    int* off = reinterpret_cast<int*>(smem + (size_t)N * 16);
    unsigned short* rev = reinterpret_cast<unsigned short*>(smem + (size_t)N * 16 + (((size_t)N * 4 + 15) & ~(size_t)15));
    int* wsum = reinterpret_cast<int*>(smem + (size_t)N * 16 + (((size_t)N * 4 + 15) & ~(size_t)15) + (((size_t)N * k * 2 + 15) & ~(size_t)15));
    const int lane = threadIdx.x & (kRegLanes - 1), sub = threadIdx.x / kRegLanes;
    constexpr int kSubs = kRegThreads / kRegLanes;
    const bool tv = a.nb && g.dfeats;
    if (tv) {
        reg_load_cloud(a.coords, b, N, pts);
        for (int i = threadIdx.x; i < N; i += kRegThreads) off[i] = 0;
        __syncthreads();
        // count: how many lists name each point
        for (int e = threadIdx.x; e < N * k; e += kRegThreads) {
            const int i = e / k, jl = reg_local(a.nb[((int64_t)b * N + i) * a.nb_ld + (e - i * k)], b, N, i);
            if (jl >= 0) atomicAdd(&off[jl], 1);
        }
        __syncthreads();
        // exclusive prefix over N <= 4 * 1024 counts: a thread owns `per` consecutive points
        const int per = (N + kRegThreads - 1) / kRegThreads, first = threadIdx.x * per;
        int mine = 0;
        for (int q = 0; q < per; ++q)
            if (first + q < N) mine += off[first + q];
        int incl = mine;
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
            const int up = __shfl_up(incl, m, 64);
            if ((int)(threadIdx.x & (kWave - 1)) >= m) incl += up;
        }
        const int wave = threadIdx.x / kWave;
        if ((threadIdx.x & (kWave - 1)) == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        int start = incl - mine;
        for (int w = 0; w < wave; ++w) start += wsum[w];
        for (int q = 0; q < per; ++q)
            if (first + q < N) {
                const int c = off[first + q];
                off[first + q] = start;
                start += c;
            }
        __syncthreads();
        // fill in arrival order: off[j] moves from the start of j's segment to its end (= the start of j + 1's)
        for (int e = threadIdx.x; e < N * k; e += kRegThreads) {
            const int i = e / k, jl = reg_local(a.nb[((int64_t)b * N + i) * a.nb_ld + (e - i * k)], b, N, i);
            if (jl >= 0) rev[atomicAdd(&off[jl], 1)] = (unsigned short)i;
        }
        __syncthreads();
        // ascending i' inside every segment (insertion sort: a segment of real neighbour lists holds a few entries)
        for (int j = threadIdx.x; j < N; j += kRegThreads) {
            const int s0 = j ? off[j - 1] : 0, s1 = off[j];
            for (int p = s0 + 1; p < s1; ++p) {
                const unsigned short v = rev[p];
                int q = p - 1;
                while (q >= s0 && rev[q] > v) {
                    rev[q + 1] = rev[q];
                    --q;
                }
                rev[q + 1] = v;
            }
        }
        __syncthreads();
    }
    for (int base = 0; base < N; base += kSubs) {
        if (base + sub >= N) continue;             // no cross-lane operation below: whole point groups may leave
        const int i = base + sub;
        const int64_t row = (int64_t)b * N + i;
        if (tv) {
            const float4 pi = pts[i];
            const float* fi = a.feats + row * a.feats_ld;
            float own[kRegChunks], acc[kRegChunks];
#pragma unroll
            for (int t = 0; t < kRegChunks; ++t) {
                const int f = lane + kRegLanes * t;
                own[t] = f < F ? fi[f] : 0.f;
                acc[t] = 0.f;
            }
            // owner part: this point's own list, in list order
            const float gi = reg_upstream(g.tv_total, g.tv_pw, row, count) * a.weight_tv;
            for (int s = 0; s < k; ++s) {
                const int jl = reg_local(a.nb[row * a.nb_ld + s], b, N, i);
                if (jl < 0) continue;
                const float c = gi * reg_inv_dist(pts[jl], pi);
                const float* fj = a.feats + ((int64_t)b * N + jl) * a.feats_ld;
#pragma unroll
                for (int t = 0; t < kRegChunks; ++t) {
                    const int f = lane + kRegLanes * t;
                    if (f < F) {
                        const float x = own[t] - fj[f];
                        acc[t] += c * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
                    }
                }
            }
            // neighbour part: every i' whose list names i, ascending i'
            const int s0 = i ? off[i - 1] : 0, s1 = off[i];
            for (int p = s0; p < s1; ++p) {
                const int o = rev[p];
                const int64_t orow = (int64_t)b * N + o;
                const float c = (reg_upstream(g.tv_total, g.tv_pw, orow, count) * a.weight_tv) * reg_inv_dist(pi, pts[o]);
                const float* fo = a.feats + orow * a.feats_ld;
#pragma unroll
                for (int t = 0; t < kRegChunks; ++t) {
                    const int f = lane + kRegLanes * t;
                    if (f < F) {
                        const float x = own[t] - fo[f];
                        acc[t] += c * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f));
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < kRegChunks; ++t) {
                const int f = lane + kRegLanes * t;
                if (f < F) g.dfeats[row * F + f] = acc[t];
            }
        }
        if (a.mean && g.dmean) {
            const float gk = reg_upstream(g.kl_total, g.kl_pw, row, count) * a.weight_kl;
            const float *m = a.mean + row * a.kl_ld, *lv = a.log_var + row * a.kl_ld;
#pragma unroll
            for (int t = 0; t < kRegChunks; ++t) {
                const int f = lane + kRegLanes * t;
                if (f < F) {
                    g.dmean[row * F + f] = gk * m[f];
                    g.dlog_var[row * F + f] = (-0.5f * gk) * (1.f - expf(lv[f]));
                }
            }
        }
    }
}

static int reg_check(const RegArgs& a, int B, int dtype) {
    if (B <= 0 || a.N <= 0 || a.F <= 0) return NPCD_ERR_ARG;
    if (!a.nb && !a.mean) return NPCD_ERR_ARG;
    if (a.nb && (!a.coords || !a.feats || a.k <= 0 || a.nb_ld < a.k || a.feats_ld < a.F)) return NPCD_ERR_ARG;
    if (a.mean && (!a.log_var || a.kl_ld < a.F)) return NPCD_ERR_ARG;
    if (dtype != NPCD_F32 || a.N > kRegMaxN || a.F > kRegMaxF || B > 65535) return NPCD_ERR_UNSUPPORTED;
    if (a.nb && (int64_t)a.k * a.N > kRegMaxPairs) return NPCD_ERR_UNSUPPORTED;
    return NPCD_OK;
}

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_stage1_reg_workspace_floats(int B) { return B > 0 ? 2 * (int64_t)B : -1; }

extern "C" int npcd_stage1_reg_fwd(const float* coords, const int32_t* nb, int64_t nb_ld, const float* feats, int64_t feats_ld, const float* mean,
                                   const float* log_var, int64_t kl_ld, int B, int N, int k, int F, float weight_tv, float weight_kl, int dtype,
                                   float* tv_pointwise, float* tv_total, float* kl_pointwise, float* kl_total, float* workspace, void* stream) {
    const RegArgs a{coords, nb, nb_ld, feats, feats_ld, mean, log_var, kl_ld, N, k, F, weight_tv, weight_kl};
    const int rc = reg_check(a, B, dtype);
    if (rc != NPCD_OK) return rc;
    if (!workspace || (nb && (!tv_pointwise || !tv_total)) || (mean && (!kl_pointwise || !kl_total))) return NPCD_ERR_ARG;
    const size_t lds = reg_fwd_lds(N);
    static DynLds lds_attr;
    if (lds > 65536) NPCD_HIP_CHECK(lds_attr.ensure(reinterpret_cast<const void*>(stage1_reg_fwd_kernel), lds));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(stage1_reg_fwd_kernel, dim3(B), dim3(kRegThreads), lds, st, a, tv_pointwise, kl_pointwise, workspace);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(stage1_reg_totals_kernel, dim3(1), dim3(kWave), 0, st, workspace, B, (float)((int64_t)B * N), nb ? tv_total : nullptr,
                       mean ? kl_total : nullptr);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_stage1_reg_bwd(const float* coords, const int32_t* nb, int64_t nb_ld, const float* feats, int64_t feats_ld, const float* mean,
                                   const float* log_var, int64_t kl_ld, int B, int N, int k, int F, float weight_tv, float weight_kl, int dtype,
                                   const float* g_tv_total, const float* g_tv_pointwise, const float* g_kl_total, const float* g_kl_pointwise,
                                   float* dfeats, float* dmean, float* dlog_var, void* stream) {
    const RegArgs a{coords, nb, nb_ld, feats, feats_ld, mean, log_var, kl_ld, N, k, F, weight_tv, weight_kl};
    const int rc = reg_check(a, B, dtype);
    if (rc != NPCD_OK) return rc;
    if ((nb && !dfeats) || (mean && (!dmean || !dlog_var))) return NPCD_ERR_ARG;
    const RegGrads g{g_tv_total, g_tv_pointwise, g_kl_total, g_kl_pointwise, dfeats, dmean, dlog_var};
    const size_t lds = nb ? reg_bwd_lds(N, k) : 0;
    static DynLds lds_attr;
    if (lds > 65536) NPCD_HIP_CHECK(lds_attr.ensure(reinterpret_cast<const void*>(stage1_reg_bwd_kernel), lds));
    hipLaunchKernelGGL(stage1_reg_bwd_kernel, dim3(B), dim3(kRegThreads), lds, static_cast<hipStream_t>(stream), a, g, (float)((int64_t)B * N));
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
