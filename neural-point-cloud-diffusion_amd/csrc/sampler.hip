// Steps of the sampler (inference; gfx950): pure streaming kernels, fp32 math, no LDS.  Roofline: HBM.
//   the DDPM reverse step per tensor (gaussian_diffusion.py:100-146 of the reference)              -> ddpm_reverse
//   a step of the scheduled sampler, both tensors in one launch, in the three forms of the C API    -> sampler_step_kernel<MASKS, HIST>
//     npcd_sampler_step           strided DDIM levels, eta, one tensor held                            <false, false>
//     npcd_sampler_step_keep      + a per-point mask that keeps some points (completion, local edits)  <true, false>
//     npcd_sampler_step_multistep the deterministic step in second order, with the previous step's
//                                 data prediction as history (DPM-Solver++ 2M), masks optional         <true, true>
#include "common.h"

namespace npcd {

// DDPM reverse step (gaussian_diffusion.py:100-146 of the reference): x0 = a x_t - b eps (clamped), mean = c1 x0 + c2 x_t,
// x_{t-1} = mean + [t > 0] exp(logvar / 2) noise; the five per-sample coefficients are looked up from the 1000-entry tables.
struct DdpmTables {
    const float *recip, *recipm1, *c1, *c2, *logvar;
};
template <class EPS>
__global__ __launch_bounds__(256) void ddpm_reverse_kernel(const float* __restrict__ x_t, const EPS* __restrict__ eps, const float* __restrict__ noise,
                                                           float* __restrict__ x_prev, float* __restrict__ x0_out, const int64_t* __restrict__ t,
                                                           int64_t per_sample, DdpmTables tab, float lo, float hi, int has_clip) {
    const int b = blockIdx.y;
    const int64_t ts = t[b];
    const float a = tab.recip[ts], bb = tab.recipm1[ts], c1 = tab.c1[ts], c2 = tab.c2[ts];
    const float sd = ts != 0 ? expf(0.5f * tab.logvar[ts]) : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * 256) {
        const int64_t j = (int64_t)b * per_sample + i;
        const float x = x_t[j];
        float x0 = a * x - bb * (float)eps[j];
        if (has_clip) x0 = fminf(fmaxf(x0, lo), hi);
        if (x0_out) x0_out[j] = x0;
        x_prev[j] = (c1 * x0 + c2 * x) + sd * noise[j];
    }
}

// Scheduled sampler step: ONE launch advances both tensors of a step, blockIdx.z = 0 coords, 1 feats, blockIdx.y = sample.  The
// coefficients of a sample are one 32-byte row of the [T, 8] table, indexed by the timestep itself
// (GaussianDiffusion.sampling_schedule; w is 0 outside SamplingSchedule.multistep_table).  A timestep outside [0, T) reads no row and
// gives NaN outputs.  Per element, by what the tensor is in this launch:
//   reverse: x0 = clamp(r x - m eps) (the expression of ddpm_reverse_kernel: the same bits),
//            D = (w == 0) ? x0 : fma(w, x0 - hist, x0) with a history (DPM-Solver++ 2M in data prediction, Lu et al. 2022), else x0,
//            out = (c1 D + c2 x) [+ s z],  x0_out = hist = x0
//   hold   : out = h1 known + h2 z       (the known tensor, forward-noised to the level the step arrives at); nothing else is written
//   masked : tensors are [B, channels, n_points], the mask one byte per point of the sample.  Every element computes both parents with
//            their own expressions and SELECTS: kept points take the hold expression, free points the reverse step (clip and x0 are
//            theirs alone; x0_out and hist of a kept point are `known`).  A select, never a blend: what is loaded for the branch not
//            taken (NaN included) does not reach an output.
// The s z term: an unmasked reverse tensor adds it iff its noise pointer is given (eta = 0: every s is 0, nothing is read), a masked
// one iff the launch is not `det`, a launch with history never.  A sample with w = 0 -- the first step, which has no history, and the
// step to the data -- loads nothing from `hist`; the branch is uniform over the workgroup (one sample, one w).  Every lane reads and
// then overwrites its own elements of `hist`, which no other lane touches.
struct SamplerCoef {
    float r, m, c1, c2, s, h1, h2, w;
};
struct SamplerTensorArgs {
    NpcdSamplerTensor rec;
    float* hist;                     // [B, per_sample]; null without history and for a hold-mode tensor
    const uint8_t* keep;             // [B, n_points] or null: the tensor goes by its mode
    int vec;                         // 16-byte items
};
struct SamplerArgs {
    SamplerTensorArgs tz[2];
    int64_t n_points;
    int det;
};
enum SamplerKind { kReverse, kHold, kMasked };

// the coefficients of sample b: its table row, or NaN for a timestep outside [0, T)
__device__ __forceinline__ SamplerCoef sampler_coef(const int64_t* __restrict__ t, const float* __restrict__ table, int T, int b) {
    const int64_t ts = t[b];
    const float nan = __builtin_nanf("");
    SamplerCoef k{nan, nan, nan, nan, nan, nan, nan, nan};
    if (ts >= 0 && ts < T) {
        const f32x4 lo = reinterpret_cast<const f32x4*>(table)[2 * ts], hi = reinterpret_cast<const f32x4*>(table)[2 * ts + 1];
        k = SamplerCoef{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    return k;
}

// An item is N consecutive elements of every operand: N = 4 moves 16 bytes per lane (8 of a bf16 eps, the four mask bytes of its four
// points as one dword: n_points % 4 == 0, so an item never straddles a channel row), N = 1 one element.  Both widths run the same
// element function below, so they give the same bits.
template <int N, class E>
__device__ __forceinline__ void item_load(const E* __restrict__ p, int64_t i, float (&v)[N]) {
    if constexpr (N == 4) {
        const f32x4 r = to_f32(reinterpret_cast<const typename V<E>::x4*>(p)[i]);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = r[q];
    } else {
        v[0] = (float)p[i];
    }
}
template <int N>
__device__ __forceinline__ void item_store(float* __restrict__ p, int64_t i, const float (&v)[N]) {
    if constexpr (N == 4) reinterpret_cast<f32x4*>(p)[i] = f32x4{v[0], v[1], v[2], v[3]};
    else p[i] = v[0];
}
// the index of item i within its channel row of n items, taken in 32 bits when it fits
__device__ __forceinline__ int64_t sampler_col(int64_t i, int64_t n) {
    return ((uint64_t)(i | n) >> 32) == 0 ? (int64_t)((uint32_t)i % (uint32_t)n) : i % n;
}
// the mask bytes of the points of item i, byte q = element q
template <int N>
__device__ __forceinline__ uint32_t item_mask(const uint8_t* __restrict__ keep, int64_t i, int64_t n_points) {
    const int64_t col = sampler_col(i, n_points / N);
    if constexpr (N == 4) return reinterpret_cast<const uint32_t*>(keep)[col];
    else return keep[col];
}

// The roundings are written out (fused multiply-adds), so that x0 is what ddpm_reverse_kernel's `a * x - bb * eps` compiles to:
// fma(a, x, -(bb eps)).  x0: 2 roundings; D: the subtraction and its fma; out: c2 x, its fma, the noise fma; hold: 2.
__device__ __forceinline__ float sampler_x0(const SamplerCoef& k, float x, float e, int has_clip, float lo, float hi) {
    float x0 = __builtin_fmaf(k.r, x, -(k.m * e));
    if (has_clip) x0 = fminf(fmaxf(x0, lo), hi);
    return x0;
}

template <SamplerKind KIND>
__device__ __forceinline__ void sampler_element(const SamplerCoef& k, const NpcdSamplerTensor& a, bool first_order, bool add_noise, float x, float e,
                                                float z, float kn, float h, bool kept, float& out, float& x0) {
    const float held = __builtin_fmaf(k.h1, kn, k.h2 * z);
    if constexpr (KIND == kHold) {
        out = held;
    } else {
        const float f0 = sampler_x0(k, x, e, a.has_clip, a.clip_lo, a.clip_hi);
        const float d = first_order ? f0 : __builtin_fmaf(k.w, f0 - h, f0);
        float fo = __builtin_fmaf(k.c1, d, k.c2 * x);
        if (add_noise) fo = __builtin_fmaf(k.s, z, fo);
        x0 = KIND == kMasked && kept ? kn : f0;
        out = KIND == kMasked && kept ? held : fo;
    }
}

// sample b of one tensor: the workgroups of the sample stride over its items
// (blocks of the wider tensor's grid that lie past this tensor's range fall through the loop)
template <SamplerKind KIND, bool HIST, class EPS, int N>
__device__ __forceinline__ void sampler_items(const SamplerTensorArgs& ta, int64_t n_points, int det, const SamplerCoef& k, int b) {
    const NpcdSamplerTensor& a = ta.rec;
    constexpr bool kSteps = KIND != kHold, kHolds = KIND != kReverse;   // elements that (may) take the reverse step / the hold expression
    const bool add_noise = !HIST && (KIND == kMasked ? !det : a.noise != nullptr);
    const bool first_order = !(HIST && kSteps) || k.w == 0.f;
    const bool reads_noise = kHolds || add_noise;
    const int64_t base = (int64_t)b * a.per_sample;
    const float* __restrict__ x_t = kSteps ? a.x_t + base : nullptr;
    const EPS* __restrict__ eps = kSteps ? static_cast<const EPS*>(a.eps) + base : nullptr;
    const float* __restrict__ noise = reads_noise ? a.noise + base : nullptr;
    const float* __restrict__ known = kHolds ? a.known + base : nullptr;
    const uint8_t* __restrict__ keep = KIND == kMasked ? ta.keep + (int64_t)b * n_points : nullptr;
    float* __restrict__ hist = HIST && kSteps ? ta.hist + base : nullptr;
    float* __restrict__ x0_out = kSteps && a.x0_out ? a.x0_out + base : nullptr;
    float* __restrict__ out = a.out + base;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.per_sample / N; i += (int64_t)gridDim.x * 256) {
        float x[N] = {}, e[N] = {}, z[N] = {}, kn[N] = {}, h[N] = {}, x0[N] = {}, o[N];
        uint32_t m = 0;
        if constexpr (KIND == kMasked) m = item_mask<N>(keep, i, n_points);
        if constexpr (kSteps) {
            item_load<N>(x_t, i, x);
            item_load<N>(eps, i, e);
        }
        if (!first_order) item_load<N>(hist, i, h);
        if (reads_noise) item_load<N>(noise, i, z);
        if constexpr (kHolds) item_load<N>(known, i, kn);
#pragma unroll
        for (int q = 0; q < N; ++q)
            sampler_element<KIND>(k, a, first_order, add_noise, x[q], e[q], z[q], kn[q], h[q], ((m >> (8 * q)) & 0xffu) != 0, o[q], x0[q]);
        if constexpr (kSteps) {
            if (x0_out) item_store<N>(x0_out, i, x0);
            if constexpr (HIST) item_store<N>(hist, i, x0);
        }
        item_store<N>(out, i, o);
    }
}

template <SamplerKind KIND, bool HIST, class EPS>
__device__ __forceinline__ void sampler_by_width(const SamplerTensorArgs& ta, int64_t n_points, int det, const SamplerCoef& k, int b) {
    if (ta.vec) sampler_items<KIND, HIST, EPS, 4>(ta, n_points, det, k, b);
    else sampler_items<KIND, HIST, EPS, 1>(ta, n_points, det, k, b);
}
template <SamplerKind KIND, bool HIST>
__device__ __forceinline__ void sampler_by_eps(const SamplerTensorArgs& ta, int64_t n_points, int det, const SamplerCoef& k, int b) {
    if (ta.rec.eps_dtype == NPCD_F32) sampler_by_width<KIND, HIST, float>(ta, n_points, det, k, b);
    else sampler_by_width<KIND, HIST, __bf16>(ta, n_points, det, k, b);
}

// MASKS / HIST: the launch may carry masks / carries history; without them that code is not in the kernel
template <bool MASKS, bool HIST>
__global__ __launch_bounds__(256) void sampler_step_kernel(SamplerArgs args, const int64_t* __restrict__ t, const float* __restrict__ table, int T) {
    const SamplerTensorArgs& ta = args.tz[blockIdx.z];
    const int b = blockIdx.y;
    const SamplerCoef k = sampler_coef(t, table, T, b);
    if (MASKS && ta.keep) sampler_by_eps<kMasked, HIST>(ta, args.n_points, args.det, k, b);
    else if (ta.rec.mode == NPCD_SAMPLER_HOLD) sampler_by_width<kHold, false, float>(ta, 0, 0, k, b);
    else sampler_by_eps<kReverse, HIST>(ta, 0, 0, k, b);
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_ddpm_reverse_step(const float* x_t, const void* eps, int eps_dtype, const float* noise, float* x_prev, float* x0_out,
                                      const int64_t* t, int B, int64_t per_sample, const float* tab_recip, const float* tab_recipm1,
                                      const float* tab_coef1, const float* tab_coef2, const float* tab_logvar, float clip_lo, float clip_hi,
                                      int has_clip, void* stream) {
    if (!x_t || !eps || !noise || !x_prev || !t || B <= 0 || per_sample <= 0) return NPCD_ERR_ARG;
    if (!tab_recip || !tab_recipm1 || !tab_coef1 || !tab_coef2 || !tab_logvar) return NPCD_ERR_ARG;
    if (eps_dtype != NPCD_F32 && eps_dtype != NPCD_BF16) return NPCD_ERR_UNSUPPORTED;
    const DdpmTables tab{tab_recip, tab_recipm1, tab_coef1, tab_coef2, tab_logvar};
    const int gx = (int)((per_sample + 255) / 256 < 1024 ? (per_sample + 255) / 256 : 1024);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (eps_dtype == NPCD_F32)
        hipLaunchKernelGGL(ddpm_reverse_kernel<float>, dim3(gx, B), dim3(256), 0, st, x_t, static_cast<const float*>(eps), noise, x_prev, x0_out, t,
                           per_sample, tab, clip_lo, clip_hi, has_clip);
    else
        hipLaunchKernelGGL(ddpm_reverse_kernel<__bf16>, dim3(gx, B), dim3(256), 0, st, x_t, static_cast<const __bf16*>(eps), noise, x_prev, x0_out, t,
                           per_sample, tab, clip_lo, clip_hi, has_clip);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

// One tensor of a scheduled step: refuses a missing or unsupported operand, then takes 16-byte items when the element counts are
// multiples of 4 and every pointer that the tensor's path touches is 16-byte aligned (8 bytes of a bf16 eps, 4 of the mask).
// `hist` is looked at only in a launch with history; a mask implies n_points > 0 (the entries see to it).
static int sampler_prepare(const NpcdSamplerTensor& a, const uint8_t* keep, float* hist, bool with_hist, int64_t n_points, int deterministic,
                           SamplerTensorArgs* ta) {
    const bool masked = keep != nullptr, hold = !masked && a.mode == NPCD_SAMPLER_HOLD;
    if (!masked && !hold && a.mode != NPCD_SAMPLER_REVERSE) return NPCD_ERR_ARG;
    const bool steps = !hold, holds = masked || hold;
    const bool reads_noise = holds || (!with_hist && a.noise);
    if (!a.out || a.per_sample <= 0 || (steps && (!a.x_t || !a.eps)) || (holds && !a.known)) return NPCD_ERR_ARG;
    if (!a.noise && (holds || !deterministic)) return NPCD_ERR_ARG;
    if (masked && a.per_sample % n_points != 0) return NPCD_ERR_ARG;
    if (steps && a.eps_dtype != NPCD_F32 && a.eps_dtype != NPCD_BF16) return NPCD_ERR_UNSUPPORTED;
    if (with_hist && steps && !hist) return NPCD_ERR_ARG;
    bool vec = a.per_sample % 4 == 0 && al16(a.out) && (!reads_noise || al16(a.noise)) && (!holds || al16(a.known));
    if (steps)
        vec = vec && al16(a.x_t) && (reinterpret_cast<uintptr_t>(a.eps) & (a.eps_dtype == NPCD_F32 ? 15 : 7)) == 0 &&
              (!a.x0_out || al16(a.x0_out)) && (!with_hist || al16(hist));
    if (masked) vec = vec && n_points % 4 == 0 && (reinterpret_cast<uintptr_t>(keep) & 3) == 0;
    *ta = SamplerTensorArgs{a, with_hist && steps ? hist : nullptr, keep, vec ? 1 : 0};
    return NPCD_OK;
}

// The launch behind the three entries.  Grid: the rule of ddpm_reverse_kernel over the items of the wider tensor -- one sweep of 256
// lanes per workgroup, at most 1024 workgroups per sample, the rest strided.
template <bool MASKS, bool HIST>
static int sampler_launch(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, float* hist_coords, float* hist_feats,
                          const uint8_t* keep_coords, const uint8_t* keep_feats, int64_t n_points, const int64_t* t, const float* table, int T,
                          int B, int deterministic, void* stream) {
    if (!coords || !feats || !t || !table || T <= 0 || B <= 0) return NPCD_ERR_ARG;
    if (B > 65535 || !al16(table)) return NPCD_ERR_UNSUPPORTED;
    SamplerArgs args;
    args.n_points = n_points;
    args.det = deterministic ? 1 : 0;
    int gx = 1;
    for (int z = 0; z < 2; ++z) {
        const NpcdSamplerTensor& a = z ? *feats : *coords;
        const int rc = sampler_prepare(a, z ? keep_feats : keep_coords, z ? hist_feats : hist_coords, HIST, n_points, deterministic, &args.tz[z]);
        if (rc != NPCD_OK) return rc;
        const int64_t sweeps = ((args.tz[z].vec ? a.per_sample / 4 : a.per_sample) + 255) / 256;
        const int g = (int)(sweeps < 1024 ? sweeps : 1024);
        gx = g > gx ? g : gx;
    }
    hipLaunchKernelGGL((sampler_step_kernel<MASKS, HIST>), dim3(gx, B, 2), dim3(256), 0, static_cast<hipStream_t>(stream), args, t, table, T);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_sampler_step(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, const int64_t* t, const float* table, int T,
                                 int B, int deterministic, void* stream) {
    return sampler_launch<false, false>(coords, feats, nullptr, nullptr, nullptr, nullptr, 0, t, table, T, B, deterministic, stream);
}

extern "C" int npcd_sampler_step_keep(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, const uint8_t* keep_coords,
                                      const uint8_t* keep_feats, int64_t n_points, const int64_t* t, const float* table, int T, int B,
                                      int deterministic, void* stream) {
    if (n_points <= 0) return NPCD_ERR_ARG;
    return sampler_launch<true, false>(coords, feats, nullptr, nullptr, keep_coords, keep_feats, n_points, t, table, T, B, deterministic, stream);
}

extern "C" int npcd_sampler_step_multistep(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, float* hist_coords,
                                           float* hist_feats, const uint8_t* keep_coords, const uint8_t* keep_feats, int64_t n_points,
                                           const int64_t* t, const float* table, int T, int B, void* stream) {
    if ((keep_coords || keep_feats) && n_points <= 0) return NPCD_ERR_ARG;
    // the schedule is deterministic: a reverse tensor needs no noise
    return sampler_launch<true, true>(coords, feats, hist_coords, hist_feats, keep_coords, keep_feats, n_points, t, table, T, B, 1, stream);
}
