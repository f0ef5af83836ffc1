// The issue ceilings of the vector ALU for plain fp32 and fp64 multiplies and adds, measured: every lane runs kChains independent chains
// of x = x * c, x = x + d (no fused multiply-add: compile with -ffp-contract=off), long enough that nothing else counts.  Prints one
// JSON line with the lane-operations per second of either format.  What tools/probes/gpu_dev_raycast.py holds the pair loop of
// csrc/raycast.hip against (docs/experiments.md R37).
//
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize tools/probes/valu_rate_probe.hip -o valu_rate_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

constexpr int kChains = 8, kThreads = 256, kBlocks = 256 * 8, kIters = 1 << 18;

template <class T>
__global__ __launch_bounds__(kThreads) void chains(T* out, int iters, T c, T d) {
    T x[kChains];
    for (int k = 0; k < kChains; ++k) x[k] = (T)(threadIdx.x + k) * (T)0.001;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < kChains; ++k) {
            x[k] = x[k] * c;
            x[k] = x[k] + d;
        }
    }
    T sum = 0;
    for (int k = 0; k < kChains; ++k) sum += x[k];
    out[(size_t)blockIdx.x * kThreads + threadIdx.x] = sum;          // kBlocks * kThreads entries
}

#define CHECK(e)                                                                 \
    do {                                                                         \
        if ((e) != hipSuccess) {                                                 \
            std::fprintf(stderr, "%s failed: %s\n", #e, hipGetErrorString(e));   \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

template <class T>
static double rate() {
    T* out;
    CHECK(hipMalloc(&out, sizeof(T) * kBlocks * kThreads));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    float best = 1e30f;
    for (int r = 0; r < 4; ++r) {          // the first is the warm-up
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL(chains<T>, dim3(kBlocks), dim3(kThreads), 0, 0, out, kIters, (T)0.999999, (T)1e-6);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (r > 0 && ms < best) best = ms;
    }
    CHECK(hipFree(out));
    return (double)kBlocks * kThreads * kIters * kChains * 2 / (best * 1e-3);
}

int main() {
    const double f32 = rate<float>(), f64 = rate<double>();
    std::printf("{\"fp32_lane_ops_per_second\": %.4g, \"fp64_lane_ops_per_second\": %.4g}\n", f32, f64);
    return 0;
}
