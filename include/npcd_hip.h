/*
 * npcd_hip.h -- C ABI of libnpcd_hip.so, the MI355X (gfx950) implementation of the NPCD hot path.
 *
 * These entry points are what the reference's two native plug points bind to
 * (paths relative to lmb-freiburg/neural-point-cloud-diffusion @ 2024_10_08):
 *
 *   flash_attn.flash_attn_func       called at npcd/models/diffusion/denoisers/transformer.py:75
 *                                    (import :9-12)                     -> npcd_attn_fwd / npcd_attn_bwd
 *   torch_knnquery.VoxelGrid         ctor  npcd/models/pointnerf/pointnerf.py:20,147-153
 *     .set_pointset                  pointnerf.py:67-75,116-124        -> npcd_grid_build
 *     .query                         fields/aggregators/aggregator.py:63 -> npcd_grid_query
 *
 * plus the fused replacements of the PyTorch op chains around them on the render path
 * (ray generation, neighbour gather + positional encoding + MLP shading, ray marching) and the
 * elementwise chains of the denoiser training step (LayerNorm, bias+GELU, q_sample/MSE, AdamW+EMA).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all buffers
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and never synchronise
 *   - return value: 0 on success, a negative NPCD_ERR_* otherwise (no exceptions cross the ABI)
 *   - strides are in ELEMENTS, the innermost (head_dim / channel) dimension is contiguous
 *   - dtype codes: NPCD_BF16 = 0, NPCD_F16 = 1, NPCD_F32 = 2, NPCD_F64 = 3 (feature statistics only)
 */
#ifndef NPCD_HIP_H
#define NPCD_HIP_H

#include <assert.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPCD_OK 0
#define NPCD_ERR_ARG (-1)          /* bad argument (null pointer, misaligned, negative size) */
#define NPCD_ERR_UNSUPPORTED (-2)  /* shape / dtype not implemented by the kernels           */
#define NPCD_ERR_HIP (-3)          /* a HIP runtime call failed (see npcd_last_hip_error)     */

#define NPCD_BF16 0
#define NPCD_F16 1
#define NPCD_F32 2
#define NPCD_F64 3

int npcd_abi_version(void);
const char* npcd_error_string(int code);
const char* npcd_last_hip_error(void);

/* ------------------------------------------------------------------------------------------
 * Attention over points: out = softmax(q k^T * scale) v, non-causal, no mask, no dropout.
 * Replaces flash_attn_func(q, k, v, causal=False, dropout_p=0) (transformer.py:75) and its
 * autograd backward.  Every entry point takes one argument block; a member an entry point does not use is ignored.
 * ------------------------------------------------------------------------------------------ */
typedef struct npcd_attn_args {
    /* q/k/v: [B, n, H, d] views (typically of one interleaved [B,n,H,3d] buffer, transformer.py:71-72) sharing the qkv strides */
    const void *q, *k, *v;
    void* out;        /* [B, n, H, d]: written by the forwards, read by the backwards */
    float* lse;       /* [B, H, n] fp32, log(sum_j exp(scale * <q_i, k_j>)): written by the forwards, read by the backwards */
    const void* dout; /* out's strides */
    void *dq, *dk, *dv;  /* share the g strides */
    /* fp32 scratch of npcd_attn_bwd_workspace_floats(B, n, H) elements, written by the backward.  First [2, B, H, npad] (npad = n
     * rounded up to a multiple of 64): the per-row constants the dK/dV pass starts its accumulators from, plane 0 = -lse / scale,
     * plane 1 = -rowsum(dout * out), pad rows -inf / 0.  Behind them, for sequences of 128 j + 1 tokens (the denoiser's 512 points +
     * timestep token): 192 floats per (batch, head, 32-row block), the partial sums of the last token's dK / dV / dQ rows (that
     * token gets no workgroup of its own; csrc/attention.hip, 'the edge token').  The fp32 kernels and head dims 32 / 128 use the
     * first B H n floats only, for rowsum(dout * out). */
    float* delta;
    /* NULL, or the COLUMN SUMS of the packed gradient as a by-product of npcd_attn_bwd (the bias gradient of c_qkv, transformer.py:
     * 67-72; replaces a separate npcd_colsum_dt pass over dqkv in the fused backbone).  Only for the packed layout (dk = dq + 64
     * elements, dv = dq + 128, g_sh = 192), the 16-bit types and d = 64, and dq must be given whatever `passes` says.
     * fp32 [npcd_attn_bwd_colsum_rows(B, n, H) + npcd_colsum_scratch_rows(), 3 H 64]; every wave writes the sums of the ROUNDED
     * rows it stores (fixed order); finish with npcd_colsum_finalize(colsum_part, rows, 3 H 64, out, ...). */
    float* colsum_part;
    /* scratch (uninitialised, 16-byte aligned) whose meaning belongs to the entry point:
     *   npcd_attn_fwd        NULL, or npcd_attn_fwd_workspace_floats(B, n, H) floats: the row-split scratch
     *   npcd_attn_fwd_fp8    npcd_attn_fwd_fp8_workspace_bytes(B, n, H) bytes: the e4m3 copies of k and v^T
     *   npcd_attn_bwd_fused  npcd_attn_bwd_fused_slab_floats(B, n, H) floats (0 for n <= 256: may be NULL): the running dQ */
    void* workspace;
    int64_t qkv_sb, qkv_sn, qkv_sh;  /* strides of q / k / v  */
    int64_t out_sb, out_sn, out_sh;  /* of out / dout         */
    int64_t g_sb, g_sn, g_sh;        /* of dq / dk / dv       */
    int32_t B, n, H, d, dtype;
    float scale;
} npcd_attn_args;
static_assert(sizeof(npcd_attn_args) == 192 && offsetof(npcd_attn_args, scale) == 188, "npcd_attn_args is part of the ABI");

/* Forward.  Head dims: d = 64 runs the specialised kernels of csrc/attention.hip; d = 32 and d = 128 (the reference's attention takes
 * any width / heads, transformer.py:68-84) run csrc/attention_gen.hip in the 16-bit types, forward and backward, and the vector-ALU
 * form of the exact fp32 FORWARD; anything else, and the fp32 backward at d != 64, is NPCD_ERR_UNSUPPORTED.
 * dtype NPCD_F32 selects the exact-fp32 kernels on the fp32 matrix instruction (the reference's fp32 sampling path,
 * diffusion_model.py:108-133, and `--dtype float32` training through its einsum attention, transformer.py:76-81): nothing is rounded
 * to 16 bits; lse is written when given (may be NULL for inference); strides multiples of 4 elements and 16-byte aligned pointers
 * take the matrix-instruction form, any other layout a vector-ALU form of the forward.
 * workspace: npcd_attn_fwd_workspace_floats is non-zero exactly when the sequence has 256 j + 1 > 256 tokens AND the 64-rows-per-wave
 * form of the forward takes it (n >= 1024, or NPCD_ATTN_FWD=64; the variable is read at every call, by the sizing function too).
 * With the scratch, that form runs without a workgroup for the last query row: the waves of each (batch, head) split that row's keys
 * and a small second kernel merges their partial softmax states. */
int64_t npcd_attn_fwd_workspace_floats(int B, int n, int H);
int npcd_attn_fwd(const npcd_attn_args* a, void* stream);

/* The same forward with fp8 (e4m3) operands on the block-scaled matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4; BASELINE
 * configs[4] names fp8 attention; opt-in, csrc/attention.hip attn_fwd_fp8_kernel): k is quantised to e4m3 and v to e4m3
 * transposed by a packing pass into `workspace`, q and P (with a 2^-8 block scale) inside the kernel.  A workspace size of 0 = this
 * length is not covered, use npcd_attn_fwd: n or n - 1 must be a multiple of 64.  bf16 only; out / lse as above;
 * the backward is npcd_attn_bwd on the bf16 operands.  Measured slower than the bf16 kernel at head_dim 64. */
int64_t npcd_attn_fwd_fp8_workspace_bytes(int B, int n, int H);
int npcd_attn_fwd_fp8(const npcd_attn_args* a, void* stream);

/* Backward of the above, two kernels.  passes: 1 = the dq pass (also writes delta), 2 = the dk/dv pass (reads delta, so pass 1 must
 * have run), 3 = both; the single passes let a caller time / schedule the two kernels separately.  NPCD_F32 is accepted as well
 * (d = 64).  Bitwise reproducible, colsum_part included. */
int64_t npcd_attn_bwd_workspace_floats(int B, int n, int H);
int npcd_attn_bwd_colsum_rows(int B, int n, int H);
int npcd_attn_bwd(const npcd_attn_args* a, int passes, void* stream);

/* Single-pass backward (csrc/attention.hip, attn_bwd_fused_kernel): the same gradients as npcd_attn_bwd from FIVE matrix products per
 * (query, key) tile instead of seven -- S and dP are formed once, dV / dK are accumulated from them with the keys on the lanes,
 * dS crosses LDS once and dQ is summed over the keys inside the matrix instruction; one workgroup per (batch, head), 256 keys per
 * pass, the running dQ between passes in `workspace`.  delta: the [2, B, H, npad] planes above (written by the kernel's prologue).
 * 16-bit types, d = 64; colsum_part is not produced.  Bitwise reproducible. */
int64_t npcd_attn_bwd_fused_slab_floats(int B, int n, int H);
int npcd_attn_bwd_fused(const npcd_attn_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * Voxel grid (torch_knnquery.VoxelGrid).  The grid description is passed by value.
 * ------------------------------------------------------------------------------------------ */
typedef struct npcd_grid_params {
    float voxel_size[3];     /* fine voxel edge lengths            (pointnerf.py:148) */
    int32_t voxel_scale[3];  /* coarse cell = fine // voxel_scale  (:149)             */
    int32_t kernel_size[3];  /* odd; dilation + candidate window   (:150)             */
    int32_t max_points_per_voxel;        /* (:151) */
    int32_t max_occ_voxels_per_example;  /* (:152) */
    float range_min[3];      /* (:153) */
    float range_max[3];
    int32_t dims[3];         /* fine grid dimensions, computed by the host */
    int32_t cdims[3];        /* coarse grid dimensions                      */
    /* Which grid the point lists, the point cap and the candidate window live on (the source of torch_knnquery is not
     * available: DESIGN.md section 3 states both readings and the evidence for each):
     *   NPCD_GRID_FINE   (0): <= max_points_per_voxel points per FINE voxel (voxel_size), candidates = the kernel_size window of
     *                         fine voxels around the sample; occupancy on the coarse grid (fine // voxel_scale), dilated by kernel_size.
     *   NPCD_GRID_SCALED (1): everything on ONE grid of edge voxel_size * voxel_scale with ceil(dims / voxel_scale) cells per
     *                         axis: point lists (<= max_points_per_voxel per cell), the max_occ_voxels cap, occupancy dilated by
     *                         kernel_size, and the kernel_size candidate window.
     * The query radius is r * max(voxel_size) -- the UNSCALED edge (aggregator.py:20) -- in both. */
    int32_t grid_level;
} npcd_grid_params;
#define NPCD_GRID_FINE 0
#define NPCD_GRID_SCALED 1

/* bytes of device workspace npcd_grid_build needs for (B, N): per point {ix,iy,iz,kept} + the
 * coarse occupancy bitmaps */
int64_t npcd_grid_workspace_bytes(const npcd_grid_params* g, int B, int N);

/* set_pointset: points [B,N,3] fp32, counts [B] int32 (points >= counts[b] are ignored). */
int npcd_grid_build(const npcd_grid_params* g, const float* points, const int32_t* counts,
                    int B, int N, void* workspace, void* stream);

/* query, dense form: x is given implicitly as ray samples x = o + depth_s * d with
 * depth_s = t0 + (s/(S-1)) * (t1 - t0) (renderer.py:49-77, volume_renderer.py:63-70), or
 * explicitly through `x` [B,R,S,3] when x != NULL (then rays_o/rays_d/t0/t1 may be NULL).
 *   mode 0 = voxel-grid semantics (DESIGN.md "VoxelGrid spec"), radius = r * max(voxel_size)
 *   mode 1 = the reference's voxel_grid=None branch (aggregator.py:42-58), radius = r
 * Outputs (dense, per ray): sample_idx [B,R,M,k] int32 (global index b*N+i sorted by
 * (dist^2, i), -1 pad), sample_loc [B,R,M,3] fp32, slot_sample [B,R,M] int32 (depth-sample
 * index of each slot, -1 = empty), nsel [B,R] int32 (selected slots per ray).            */
int npcd_grid_query(const npcd_grid_params* g, const void* workspace, const float* points,
                    int B, int N, int R, int S, int M, int k, float r, int mode,
                    const float* x, const float* rays_o, const float* rays_d,
                    const float* t0, const float* t1,
                    int32_t* sample_idx, float* sample_loc, int32_t* slot_sample, int32_t* nsel,
                    void* stream);

/* query, fused-render form (voxel-grid semantics only): COMPACT shading-point lists instead of the
 * dense [ray, slot] arrays, no host round trip.  Per ray: ray_base (row of its first valid slot in the
 * compact lists), ray_nsel, ray_bits (bit j = slot j has >= 1 neighbour).  Compact rows (slot order
 * within a ray, ray order unspecified): nb_idx [capacity,k] int32, pts [capacity,3] fp32.
 * counter [4] int32 (ABI 8; two words before): counter[0] = number of compact rows P, counter[1] != 0 if capacity was too small,
 * counter[2] = 0 (the range-guard word the caller may pass to npcd_shade_points as `status`: zeroed by this call so that the
 * guard costs no launch of its own), counter[3] = 0 (reserved). */
int npcd_grid_query_compact(const npcd_grid_params* g, const void* workspace, const float* points,
                            int B, int N, int R, int S, int M, int k, float r,
                            const float* rays_o, const float* rays_d, const float* t0, const float* t1,
                            int32_t* counter, int32_t capacity, int32_t* ray_base, int32_t* ray_nsel,
                            uint64_t* ray_bits, int32_t* nb_idx, float* pts, void* stream);

/* The same query with the compact rows laid out in RAY ORDER: the query kernel leaves each ray's rows and count in `order_ws`
 * (npcd_grid_query_order_ws_bytes(B, R, M, k) bytes of device scratch, 16-byte aligned, uninitialised), a second launch turns the
 * counts into ray_base by a prefix sum and moves the rows.  No atomics: ray_base / nb_idx / pts are bit-identical from run to run
 * (torch_knnquery.VoxelGrid.query returns its rows in ray order as well: aggregator.py:63-73 indexes them by the ray mask).
 * Rows past `capacity` are not written and counter[1] is raised; counter [4] needs no initialisation.  More than 32,768 rays per
 * call: one more small launch adds the counts up per 1,024 rays first (same bits; keeps the prefix sums linear in the rays). */
int64_t npcd_grid_query_order_ws_bytes(int B, int R, int M, int k);
int npcd_grid_query_compact_ordered(const npcd_grid_params* g, const void* workspace, const float* points,
                                    int B, int N, int R, int S, int M, int k, float r,
                                    const float* rays_o, const float* rays_d, const float* t0, const float* t1,
                                    int32_t* counter, int32_t capacity, int32_t* ray_base, int32_t* ray_nsel,
                                    uint64_t* ray_bits, int32_t* nb_idx, float* pts, void* order_ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray generation + box limits (ray_sampler.py:10-49, math_utils.py:46-97, renderer.py:36-47).
 * extr [V,4,4] world2cam fp32, intr [V,3,3] fp32 -> rays_o/rays_d [V,res*res,3], t0/t1 [V,res*res].
 * limits_ws: npcd_ray_gen_ws_floats(V, res, n_ids) floats of device scratch (n_ids = 0 for all res^2 pixels), uninitialised: the
 * call leaves the global min start / max end / hit flag in its first words, behind them the per-workgroup limits (combined without
 * atomics by the fix-up kernel).
 * ------------------------------------------------------------------------------------------ */
int64_t npcd_ray_gen_ws_floats(int V, int res, int n_ids);
int npcd_ray_gen(const float* extr, const float* intr, int V, int res, float box,
                 float* rays_o, float* rays_d, float* t0, float* t1, float* limits_ws, void* stream);
/* Same for a subset of the pixels: pixel_ids [n_ids] int32 row-major pixel numbers (i * res + j), the same for every view
 * (the training path renders ~100 random pixels per view: renderer.py:232-238) -> rays_o/rays_d [V,n_ids,3], t0/t1 [V,n_ids]. */
int npcd_ray_gen_subset(const float* extr, const float* intr, int V, int res, float box, const int32_t* pixel_ids, int n_ids,
                        float* rays_o, float* rays_d, float* t0, float* t1, float* limits_ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused shading of compact shading points (aggregators/mlp.py:36-125, fields/mlp.py:38-72,
 * field.py:113-141): gather -> rel. position -> positional encoding -> 5-layer MLP ->
 * inverse-distance aggregation -> density head (softplus(x-1)) and colour head (sigmoid).
 * Weights are packed once by npcd_shade_pack_weights into `wpack`.
 *   nb_idx [P,k] int32 (-1 pad), pts [P,3] fp32, kp_pos [B*N,3] fp32, kp_feat [B*N,F] fp32
 *   -> sigma [P] fp32, rgb [P,3] fp32.  n_points_dev: device int32 holding P (so that P may be
 *   produced on the device without a host round trip); max_points = rows allocated in every
 *   per-point array: it bounds the launch and the kernels clamp the device-side count to it.
 * Range guard (ABI 8).  The kernels carry activations between layers as fp16 (fp32 accumulation); the reference runs these MLPs in
 * fp32 (eval_pointnerf.py has no autocast).  `status` (device int32, may be NULL) is OR-ed with NPCD_SHADE_NONFINITE_PAIRS when an
 * aggregated feature row, and with NPCD_SHADE_NONFINITE_HEADS when a head's final pre-activation, is inf / NaN -- which is where
 * every fp16 overflow (|x| >= 65,520) of an earlier layer ends up.  The library never clears the word: zero it, render, read it
 * with the point count.  A set bit means the pixels of this call are not the reference's; use the fp32-class path instead.
 * ------------------------------------------------------------------------------------------ */
#define NPCD_SHADE_NONFINITE_PAIRS 1
#define NPCD_SHADE_NONFINITE_HEADS 2
int64_t npcd_shade_wpack_bytes(int feat_dim, int n_freqs, int hidden);
int64_t npcd_shade_workspace_bytes(int max_points, int hidden);
int npcd_shade_pack_weights(const float* const* weights_host, const float* const* biases_host,
                            int feat_dim, int n_freqs, int hidden, void* wpack_host);
int npcd_shade_points(const void* wpack, int feat_dim, int n_freqs, int hidden,
                      const int32_t* nb_idx, const float* pts, const float* kp_pos, const float* kp_feat,
                      const int32_t* n_points_dev, int max_points, int k,
                      float* sigma, float* rgb, void* workspace, int32_t* status, void* stream);

/* The same with the reference's use_view_dir option (models/npcd.py:8 -> fields/mlp.py:30-36,67-70): the first colour layer sees
 * [feat | enc(ray direction)].  Its direction part is the same for every shading point of a ray, so the caller passes it per RAY:
 * dir_bias [n_rays, hidden] fp32 = enc(d) . W[:, hidden:]^T (16-byte aligned), point_ray [max_points] int32 = the ray of every compact
 * row; wpack holds that layer packed from its first `hidden` columns.  Added to the fp32 accumulators of the layer. */
int npcd_shade_points_dir(const void* wpack, int feat_dim, int n_freqs, int hidden,
                          const int32_t* nb_idx, const float* pts, const float* kp_pos, const float* kp_feat,
                          const int32_t* n_points_dev, int max_points, int k,
                          float* sigma, float* rgb, void* workspace, const float* dir_bias, const int32_t* point_ray,
                          int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * The POINT-level layers in the reference's fp32 numerics class (round 5, ABI 8): last aggregator layer (linear; aggregators/mlp.py:83-84,
 * local_field[8]), shape_net + softplus(x - 1) (fields/mlp.py:38-51, field.py:30,126-128), channel_net + sigmoid (fields/mlp.py:53-72,
 * field.py:139-140) on `feat` [max_points, 256] fp32 = the aggregated per-point features (the output of npcd_pair_mlp_fwd with
 * NPCD_PAIR_MLP_X2 + the weighted mean).  Every operand is two bf16 halves, every product three matrix instructions in fp32
 * accumulators (the numerics of NPCD_PAIR_MLP_X2: ~4e-6 relative per layer, fp32's exponent range); csrc/points_x2.hip.
 *   npcd_points_x2_pack: the twelve HOST pointers of npcd_shade_pack_weights (entries 4..11 are read); c0_in_dim = input columns of
 *   channel_net.0 (256, or 256 + the direction encoding: its first 256 columns are packed).
 *   npcd_points_x2: n_points_dev may be NULL (= max_points); dir_bias [rows, 256] fp32 + point_ray [max_points] int32 add row
 *   point_ray[p] to the first colour layer's pre-activation of point p (use_view_dir, fields/mlp.py:67-70), or both NULL.
 *   -> sigma [max_points], rgb [max_points, 3] (activations applied).
 * ------------------------------------------------------------------------------------------ */
/* The four non-linear PER-PAIR layers + the inverse-distance mean in the same numerics, forward only (aggregators/mlp.py:62-125,
 * aggregator.py:122-156, positional_encoder.py:16-20): nb_idx [max_points, k] int32 global neighbour indices (-1 = none, anywhere in a
 * row: the compact query's lists as they are), pts [max_points, 3], kp_pos [B N, 3], kp_feat [B N, feat_dim] -> G [max_points, 256] fp32,
 * the input of npcd_points_x2.  feat_dim in {32, 128}, k <= 8; n_points_dev may be NULL.  npcd_pairs_x2_pack reads entries 0..3 of the
 * twelve host pointers.  (npcd_pair_mlp_fwd with NPCD_PAIR_MLP_X2 computes the same and can save its activations for training.) */
int64_t npcd_pairs_x2_wpack_bytes(int feat_dim);
int npcd_pairs_x2_pack(const float* const* weights_host, const float* const* biases_host, int feat_dim, void* wpack_host);
int npcd_pairs_x2(const void* wpack, int feat_dim, const int32_t* nb_idx, const float* pts, const float* kp_pos, const float* kp_feat,
                  const int32_t* n_points_dev, int max_points, int k, float* G, void* stream);
int64_t npcd_points_x2_wpack_bytes(void);
int npcd_points_x2_pack(const float* const* weights_host, const float* const* biases_host, int c0_in_dim, void* wpack_host);
int npcd_points_x2(const void* wpack, const float* feat, const int32_t* n_points_dev, int max_points, float* sigma, float* rgb,
                   const float* dir_bias, const int32_t* point_ray, void* stream);
/* The same layers as the stage-1 TRAINING forward (published configuration, no view directions): save [6][max_points][256] fp32 = feat, s0, c0,
 * c1, c2, c3 (every hidden activation, after its LeakyReLU where the layer has one: what the backward of the eight Linear layers
 * needs), pre [max_points][4] = the heads' pre-activations (r, g, b, sigma) with their biases -- softplus(x - 1) / sigmoid are the
 * caller's (autograd's). */
int npcd_points_x2_train(const void* wpack, const float* feat, int max_points, float* save, float* pre, void* stream);
/* npcd_points_x2_pack from DEVICE tensors (training packs once per optimizer step): weights_dev / biases_dev = a host array of the eight
 * device pointers of local_field.8, shape_net.{0,2}, channel_net.{0,2,4,6,8}. */
int npcd_points_x2_pack_dev(const float* const* weights_dev, const float* const* biases_dev, int c0_in_dim, void* wpack_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray marching (renderer.py:96-110,120-185, volume_renderer.py:23-39) on the dense slot layout:
 * sigma/rgb are COMPACT per valid slot (row-major over [ray, slot]); slot_valid [Nr,M] uint8,
 * slot_loc [Nr,M,3], point_base [Nr] int32 = index of the ray's first compact point.
 * -> mask [Nr], depth [Nr], channels [Nr,3].  depth_ws: npcd_ray_march_ws_floats(Nr) floats of scratch, uninitialised: the
 * call leaves the global depth limits in its first two words (npcd_ray_march_bwd reads them), the rest holds the per-workgroup
 * limits of the march (one wave per ray for M <= 64; combined without atomics by the clamp kernel).
 * ------------------------------------------------------------------------------------------ */
int64_t npcd_ray_march_ws_floats(int Nr);
int npcd_ray_march(const float* sigma, const float* rgb, const uint8_t* slot_valid, const float* slot_loc,
                   const int32_t* point_base, const float* rays_o, const float* rays_d, const float* t1,
                   int Nr, int M, int white_back, float* mask, float* depth, float* channels,
                   float* depth_ws, void* stream);

/* Backward of npcd_ray_march w.r.t. sigma and rgb (stage-1 training: positions and rays are constants).  depth_ws is the
 * scratch the forward call left (global depth limits); g_mask / g_depth [Nr], g_chan [Nr,3] are the upstream gradients;
 * dsigma [P], drgb [P,3] are written for every compact point.  M <= 64. */
int npcd_ray_march_bwd(const float* sigma, const float* rgb, const uint8_t* slot_valid, const float* slot_loc,
                       const int32_t* point_base, const float* rays_o, const float* rays_d, const float* t1,
                       int Nr, int M, int white_back, const float* depth_ws, const float* g_mask, const float* g_depth,
                       const float* g_chan, float* dsigma, float* drgb, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise / normalisation / optimizer kernels of the denoiser training step (HBM-bound).
 * They fuse the eager op chains of transformer.py:169-172,136-137 (under autocast) and of
 * diffusion_training.py:169-174 + utils/ema.py:114-138.  16-bit tensors are passed as void*; dtype = their type: NPCD_BF16 (bf16
 * autocast) or NPCD_F16 (float16 autocast with loss scaling -- the reference's default --dtype, train_diffusion.py:78,
 * train/diffusion_training.py:60-62).
 * ------------------------------------------------------------------------------------------ */
/* x_out = x_in (+ delta); y = LayerNorm(x_out)*gamma+beta in `dtype`; mean/rstd [T] saved.
 * delta (`dtype` [T,W]) and x_out may be NULL.  W % 4 == 0, W <= 2048. */
int npcd_add_ln_fwd_dt(const float* x_in, const void* delta, const float* gamma, const float* beta,
                       float* x_out, void* y, float* mean, float* rstd, int T, int W, float eps, int dtype, void* stream);
/* LayerNorm backward: dx = LNbwd(dy) (+ dres), optionally also in `dtype` (dxb); column partials
 * [npcd_ln_bwd_blocks(T)][W] of dgamma, dbeta and of dx (any may be NULL). */
int npcd_ln_bwd_blocks(int T);
int npcd_ln_bwd_dt(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                   const float* dres, float* dx, void* dxb, float* part_gamma, float* part_beta,
                   float* part_col, int T, int W, int dtype, void* stream);
/* out[c] (+)= sum_b part[b][c], fixed summation order.  `part` [nblk][N] must be followed by
 * npcd_colsum_scratch_rows() more rows of N floats (used as the stage buffer of the 2-stage sum). */
int npcd_colsum_scratch_rows(void);
int npcd_colsum_finalize(const float* part, int nblk, int N, float* out, int accumulate, void* stream);
/* Up to NPCD_COLSUM_MAX_JOBS independent column sums in one pair of launches (bit-identical to the single
 * call per job).  One residual block's backward emits eight: LN dgamma/dbeta x2, four Linear bias gradients
 * (the reference gets them from autograd's SumBackward nodes, transformer.py:162-172). */
#define NPCD_COLSUM_MAX_JOBS 8
typedef struct NpcdColsumJob {
    const float* part; /* [nblk + npcd_colsum_scratch_rows()][N] */
    float* out;        /* [N] */
    int nblk, N, accumulate, reserved;
} NpcdColsumJob;
int npcd_colsum_finalize_batch(const NpcdColsumJob* jobs, int njobs, void* stream);
/* GELU (exact erf form); the backward also emits column partials [npcd_colsum_blocks(T)][N] of dh, npcd_colsum_dt those of a [T, N] */
int npcd_gelu_fwd_dt(const void* h, void* g, int64_t numel, int dtype, void* stream);
int npcd_colsum_blocks(int T);
int npcd_gelu_bwd_dt(const void* dg, const void* h, void* dh, float* part, int T, int N, int dtype, void* stream);
int npcd_colsum_dt(const void* a, float* part, int T, int N, int dtype, void* stream);
/* Weight gradient of a Linear layer with J <= 4 outputs (the PointNeRF field's heads: fields/mlp.py:38-72, last layers 256 -> 1 and
 * 256 -> 3) over T rows: part [npcd_small_wgrad_blocks(T) + npcd_colsum_scratch_rows(), J * K] fp32 partial sums of
 * dW[j][k] = sum_p dy[p][j] x[p][k] (dy [T, J], x [T, K] bf16 row-major, K a power of two in 64..2048); finish with
 * npcd_colsum_finalize(part, blocks, J * K, dW, ...).  Replaces the library GEMM (350 us for one workgroup's worth of work). */
int npcd_small_wgrad_blocks(int T);
int npcd_small_wgrad(const void* dy, const void* x, float* part, int T, int J, int K, void* stream);
/* AdamW (torch semantics) + EMA lerp + 16-bit shadow copy + optional gradient zeroing, one pass.
 * ema and shadow may be NULL; shadow_dtype = the type of the 16-bit parameter shadow; step is the 1-based step count (bias correction). */
int npcd_adamw_ema_dt(float* p, float* g, float* m, float* v, float* ema, void* shadow, int shadow_dtype, int64_t numel,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      float ema_decay, int zero_grad, void* stream);
int npcd_cast_f32_dt(const float* src, void* dst, int64_t numel, int dtype, void* stream);

/* ---- loss scaling and gradient clipping on the device (the reference's GradScaler + clip_grad_norm_,
 * train/diffusion_training.py:62,156-174): the overflow check, the global norm, the skip decision, the scale
 * update and the AdamW step count live in a control record in device memory that the optimizer kernel reads,
 * so that no step waits for the GPU.  Per step:
 *   npcd_grad_stats (per gradient range, into its own slot)  [-> all-reduce(SUM) of the slots across ranks]
 *   -> npcd_scaler_finalize (reads the slots, updates the record) -> npcd_adamw_ema_gated (per range).
 *
 * Control record, 64 bytes (16 x 4-byte words), every field written by npcd_scaler_finalize only; the host
 * initialises it and may overwrite loss_scale / step / skipped between steps:
 *   word 0  found_inf       int32  1 when the last finalized gradient held an inf / nan (the step is skipped)
 *   word 1  step            int32  AdamW steps applied (t); +1 per finalize without overflow
 *   word 2  growth_tracker  int32  clean steps since the last scale change
 *   word 3  skipped         int32  steps skipped so far
 *   word 4  loss_scale      float  scale of the NEXT backward (a power of two)
 *   word 5  inv_scale       float  1 / the scale the finalized gradient carries
 *   word 6  grad_norm       float  global L2 norm of the UNSCALED gradient, +inf when it overflowed
 *   word 7  clip_coef       float  min(max_norm / (grad_norm + 1e-6), 1) (torch's formula); 1 without clipping
 *   word 8  bc1             float  (float)(1 - beta1^step), double-precision pow, as npcd_adamw_ema_dt computes it
 *   word 9  bc2_sqrt        float  (float)sqrt(1 - beta2^step)
 *   words 10-15 reserved (zero) */
typedef struct NpcdScalerCtl {
    int32_t found_inf, step, growth_tracker, skipped;
    float loss_scale, inv_scale, grad_norm, clip_coef, bc1, bc2_sqrt;
    int32_t reserved[6];
} NpcdScalerCtl;
/* Statistics of the fp32 range g[0, n): out[0] = sum of g^2 over the finite elements (fp64 accumulation), out[1] = number
 * of inf / nan elements.  `work`: 2 * npcd_grad_stats_blocks() doubles.  Two launches (per-workgroup partials, then
 * their sum in a fixed order), no atomics: the same data gives the same bits on every run.  g 16-byte aligned, any n >= 1. */
int npcd_grad_stats_blocks(void);
int npcd_grad_stats(const float* g, int64_t n, double* work, double* out, void* stream);
/* One workgroup: sums stats[0 .. nslots) in slot order, then updates the record.  scaling = 0: no loss scaling (found_inf
 * stays 0, inv_scale 1, the scale is not touched); otherwise GradScaler's dynamic scale: x backoff on overflow (step skipped,
 * growth tracker reset), x growth after growth_interval clean steps.  clip = 0: clip_coef = 1. */
int npcd_scaler_finalize(const double* stats, int nslots, NpcdScalerCtl* ctl, int scaling, int clip, float max_norm,
                         float beta1, float beta2, float growth_factor, float backoff_factor, int growth_interval, void* stream);
/* npcd_adamw_ema_dt on the gradient (g * ctl->inv_scale) * ctl->clip_coef with ctl->bc1 / ctl->bc2_sqrt as bias corrections.
 * When ctl->found_inf is set, p, m, v and the shadow are left untouched; the EMA still moves towards p (the reference updates it
 * every iteration) and g is still zeroed when zero_grad is set.  EMA weight: 1 - (float)ema_decay on an applied step (as
 * npcd_adamw_ema_dt), (float)(1 - ema_decay) on a skipped one (torch's lerp_ weight, as the host-side loss scaler moves it). */
int npcd_adamw_ema_gated(float* p, float* g, float* m, float* v, float* ema, void* shadow, int shadow_dtype, int64_t numel,
                         float lr, float beta1, float beta2, float eps, float weight_decay, double ema_decay, int zero_grad,
                         const NpcdScalerCtl* ctl, void* stream);

/* Weight gradient of a Linear layer (the nn.Linear weight gradients of transformer.py:67-72, :107-115, :118-137, which autograd
 * computes in the reference): dW [N, K] fp32 = dy[T, N]^T x[T, K], dy / x row-major in the 16-bit `dtype`, fp32 accumulation and
 * output; N % 256 == 0, K % 256 == 0, any T.  The token range is split over npcd_wgrad_slices(T, N, K) workgroup slices that write
 * fp32 slabs (`workspace`: that many x N x K floats, unused when it is 1) which a second kernel adds in slice order: bitwise
 * reproducible.  NPCD_ERR_UNSUPPORTED for other shapes (the caller then uses the library). */
int npcd_wgrad_slices(int T, int N, int K);
int npcd_wgrad(const void* dy, const void* x, float* out, float* workspace, int T, int N, int K, int dtype, void* stream);
/* (ABI 9) `count` (1..16; 1..8 before the multi-block launch) such weight gradients over the SAME token range in one launch: dW_g [N_g, K_g] = dy_g[T, N_g]^T x_g[T, K_g].
 * One workgroup per 256 x 256 output tile over all T tokens: no slices, no workspace, one fixed summation order.  Meant for the token
 * count of one rank of the strong-scaling job (T = 4,104: the four Linear layers of a block are 192 tiles = one round on 192 of 256
 * CUs, beside the backward's critical path on another stream) and for the four Linear layers of FOUR blocks at the token count of a
 * whole batch (T = 32,832: 768 tiles = three full rounds of 256 CUs).  dy / x / out / N / K: host arrays of `count` entries; the
 * `out` pointers must differ (NPCD_ERR_ARG otherwise, as for count > 16). */
int npcd_wgrad_group(int count, const void* const* dy, const void* const* x, float* const* out, const int* N, const int* K, int T,
                     int dtype, void* stream);
/* How many residual blocks of `tiles_per_block` output tiles (256 x 256) and `products_per_block` products each belong into one
 * npcd_wgrad_group launch: the smallest G >= 1 with G * products_per_block <= min(max_products, 16) whose G * tiles_per_block
 * workgroups fill whole rounds of the current device's compute units (hipDeviceGetAttribute) to at least 0.95; 0 when no G does or
 * no device answers.  256 CUs: 192 tiles (width 1,024) -> 4, 768 tiles (width 2,048) -> 1, 48 tiles (width 512) -> 0. */
int npcd_wgrad_group_blocks(int tiles_per_block, int max_products, int products_per_block);

/* Linear layers of the residual block as own NT products with fused epilogues (csrc/gemm_nt.hip): 16-bit `dtype` operands
 * (NPCD_BF16 / NPCD_F16), fp32 accumulation, 16-bit outputs; x [M, K], w [N, K] row-major (the nn.Linear weight as stored), any
 * M >= 1, N % 1024 == 0, K % 64 == 0, M * N and M * K below 2^31, pointers 16-byte aligned; NPCD_ERR_UNSUPPORTED otherwise (the
 * caller then uses the library).  Replace, in the reference, F.linear of transformer.py:67 / :107-115 / :118-137 and the autograd
 * nodes behind them:
 *   npcd_linear_fwd:        y = x w^T + bias                                   (bias [N] 16 bit, may be NULL)
 *   npcd_linear_gelu_fwd:   h = x w^T + bias (rounded to 16 bit), g = gelu_erf(h)   -- mlp.c_fc followed by nn.GELU() (:131)
 *   npcd_linear_dgelu_bwd:  dh = round16(dy wt^T) * gelu_erf'(h)               -- the data gradient of mlp.c_proj (wt = its weight
 *                           TRANSPOSED, [N = 4 W, K = W] row-major, npcd_transpose_16) followed by the GELU backward; also writes
 *                           part [npcd_linear_dgelu_rows(M)][N] fp32 column partial sums of dh (the c_fc bias gradient), to be
 *                           finished by npcd_colsum_finalize(part, npcd_linear_dgelu_rows(M), N, ...)
 * A data gradient dx = dy W is npcd_linear_fwd(dy, W^T, NULL, ...). */
int npcd_linear_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int dtype, void* stream);
int npcd_linear_gelu_fwd(const void* x, const void* w, const void* bias, void* h, void* g, int M, int N, int K, int dtype, void* stream);
int npcd_linear_dgelu_rows(int M);
int npcd_linear_dgelu_bwd(const void* dy, const void* wt, const void* h, void* dh, float* part, int M, int N, int K, int dtype, void* stream);
/* The same product y = x w^T + bias on 128 x 128 tiles (csrc/gemm_nt.hip, lin128_kernel): the form for the token counts of ONE RANK
 * of the strong-scaling job (T = 4,104 / 8,208 per rank at 8 / 4 GPUs), where the N = 1,024 products of a block are 64-68 tiles of
 * 256 x 256 on 256 CUs.  Any M >= 1 (left-over rows M mod 128 <= 32 ride on the last row tile), N % 128 == 0, K % 64 == 0, M * K and
 * N * K below 2^30 elements (32-bit byte offsets), M * N below 2^31; 16-byte aligned pointers. */
int npcd_linear128_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int dtype, void* stream);
/* out [C, R] = in [R, C]^T for 16-bit elements (the transposed shadow of the Linear weights that the data gradients read) */
int npcd_transpose_16(const void* in, void* out, int R, int C, void* stream);
/* `count` (1..4) such transposes in ONE launch: out_g [C_g, R_g] = in_g [R_g, C_g]^T, 16-bit elements of any type (the four Linear
 * weights of a residual block -> the transposed shadow that the data-gradient products read).  16 bytes per lane on loads and
 * stores where a side's pointer and row pitch are 16-byte aligned, 2 bytes per lane on that side otherwise and at ragged edges:
 * any R, C >= 1, pointers 2-byte aligned.  in / out / R / C: host arrays of `count` entries; in and out must not overlap. */
int npcd_transpose16_group(int count, const void* const* in, void* const* out, const int* R, const int* C, void* stream);

/* out[i] = part[0 * numel + i] + ... + part[(S - 1) * numel + i], fp32, added in slice order (S = 2, 4 or 8; numel % 4 == 0;
 * 16-byte aligned): the sum of the row-split weight-gradient partials of the fused backbone (replaces torch.sum(part, dim=0)
 * there; the reference's nn.Linear weight gradient, summed over token slices). */
int npcd_sum_slices(const float* part, float* out, int S, int64_t numel, void* stream);

/* One DDPM reverse step of the sampler, fused (reference gaussian_diffusion.py:100-146: _predict_xstart_from_eps :127-129,
 * clamp :111-113, posterior mean :88-98, noise add :138-144):
 *   x0 = recip[t] x_t - recipm1[t] eps (clamped to [clip_lo, clip_hi] if has_clip); x_prev = coef1[t] x0 + coef2[t] x_t
 *        + [t > 0] exp(logvar[t] / 2) noise.
 * x_t, noise, x_prev (and x0_out, may be NULL) are fp32 [B, per_sample]; eps is fp32 or bf16 (eps_dtype); t is int64 [B];
 * the five tables are the process's fp32 [num_timesteps] device arrays. */
int npcd_ddpm_reverse_step(const float* x_t, const void* eps, int eps_dtype, const float* noise, float* x_prev, float* x0_out,
                           const int64_t* t, int B, int64_t per_sample, const float* tab_recip, const float* tab_recipm1,
                           const float* tab_coef1, const float* tab_coef2, const float* tab_logvar, float clip_lo, float clip_hi,
                           int has_clip, void* stream);

/* One step of the SCHEDULED sampler (strided DDIM schedule with eta in [0, 1]; replacement conditioning), both tensors of the step
 * (coords, feats) in ONE launch.  `table` is fp32 [T, 8] on the device, one 32-byte row per level, indexed by the timestep itself:
 * (r, m, c1, c2, s, h1, h2, 0), built by GaussianDiffusion.sampling_schedule (rows of levels that are not on the schedule are NaN;
 * a timestep outside [0, T) reads no row and gives NaN).  Per tensor, with its own per_sample (fp32 [B, per_sample] throughout):
 *   mode NPCD_SAMPLER_REVERSE: x0 = r[t] x_t - m[t] eps (clamped to [clip_lo, clip_hi] if has_clip; the same bits as the x0 of
 *        the reverse step above on the same r, m), out = (c1[t] x0 + c2[t] x_t) + s[t] noise.  eps is fp32 or bf16 (eps_dtype).
 *        noise may be NULL only when `deterministic` is non-zero (the caller's statement that every s of the table is 0, eta = 0):
 *        the term is then skipped and nothing is read.  x0_out receives x0 when not NULL.  known is ignored.
 *   mode NPCD_SAMPLER_HOLD   : out = h1[t] known + h2[t] noise (the known tensor forward-noised to the level the step arrives at;
 *        exactly known on the last step, h1 = 1 and h2 = 0).  known and noise must be given; x_t, eps, x0_out and the clip are ignored.
 * t is int64 [B], shared by both tensors.  Pointers are 4-byte aligned (2 bytes for bf16 eps); a tensor whose per_sample is a
 * multiple of 4 and whose pointers are 16-byte aligned (8 bytes for bf16 eps) moves 16 bytes per lane.  No atomics: the same bits
 * on every run.  NPCD_ERR_ARG for a missing pointer (a NULL noise without `deterministic` included) or a bad mode, NPCD_ERR_UNSUPPORTED
 * for another eps_dtype or B above 65535, before any launch. */
#define NPCD_SAMPLER_REVERSE 0
#define NPCD_SAMPLER_HOLD 1
typedef struct NpcdSamplerTensor {
    const float* x_t;
    const void* eps;
    const float* noise;
    const float* known;
    float* out;
    float* x0_out;
    int64_t per_sample;
    float clip_lo, clip_hi;
    int32_t has_clip, mode, eps_dtype, reserved;
} NpcdSamplerTensor;
int npcd_sampler_step(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, const int64_t* t, const float* table, int T,
                      int B, int deterministic, void* stream);

/* The same step with per-point keeping (completion, local edits).  Tensors are fp32 [B, channels, n_points] with the point index
 * fastest (what the denoiser takes; per_sample = channels * n_points); keep_coords / keep_feats are bytes [B, n_points], non-zero =
 * the point is kept, shared by all channels of the tensor.
 *   mask NULL : that tensor follows its `mode` exactly as in npcd_sampler_step (the same bits).
 *   mask given: x_t, eps, noise and known must all be given; `mode` is ignored; n_points must divide per_sample.  Per element of
 *        point p:  out = keep[b, p] ? h1[t] known + h2[t] noise : (the reverse step of npcd_sampler_step),
 *        the kept branch with the bits of NPCD_SAMPLER_HOLD and the free branch with the bits of NPCD_SAMPLER_REVERSE on the same
 *        operands.  The clip and x0 belong to free points; x0_out (may be NULL) receives `known` at kept points.  The branches are
 *        SELECTED, not blended: `known` at free points and x_t / eps at kept points may hold anything, NaN included, and do not
 *        reach an output.  With `deterministic` non-zero the s[t] noise term of free points is skipped, as a reverse tensor without
 *        noise skips it; the noise is still required, for the kept points.
 * Both tensors go in ONE launch on the grid rule of npcd_sampler_step (at most 1024 workgroups per sample and tensor); no atomics: the
 * same bits on every run.  A masked tensor moves 16 bytes per lane, and reads the four mask bytes of its four points at once, when
 * n_points is a multiple of 4, the mask pointer is 4-byte aligned and its pointers are 16-byte aligned (8 bytes for bf16 eps);
 * otherwise one element per lane.  NPCD_ERR_ARG for a missing operand, n_points <= 0 or a per_sample of a masked tensor that n_points
 * does not divide; NPCD_ERR_UNSUPPORTED as for npcd_sampler_step; both before any launch. */
int npcd_sampler_step_keep(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, const uint8_t* keep_coords,
                           const uint8_t* keep_feats, int64_t n_points, const int64_t* t, const float* table, int T, int B,
                           int deterministic, void* stream);

/* The deterministic step in second order: DPM-Solver++(2M) in data prediction (Lu et al. 2022) on the levels of the schedule.
 * `table` is SamplingSchedule.multistep_table: the eta = 0 table of npcd_sampler_step with the multistep weight w in column 7,
 * (r, m, c1, c2, 0, h1, h2, w).  Per element of a reverse-mode tensor, or of a free point of a masked one:
 *   x0 = r[t] x_t - m[t] eps (clamped if has_clip: the bits of npcd_sampler_step's x0),
 *   D  = w[t] == 0 ? x0 : fma(w[t], x0 - hist, x0),   out = fma(c1[t], D, c2[t] x_t),   hist = x0.
 * hist_coords / hist_feats are fp32 [B, per_sample], the previous step's x0 of that tensor; every element is read (only where
 * w[t] != 0) and then overwritten in place by the lane that owns it.  A sample whose row has w = 0 (the first step of a run, which
 * has no history, and the step to the data) reads nothing from `hist` -- it may be uninitialised or NaN -- and its out has the bits
 * of NPCD_SAMPLER_REVERSE with `deterministic` on the same operands.  The clip applies to x0 before the extrapolation; the stored
 * history and x0_out are the clipped x0.  There is no noise term: the noise of a reverse-mode tensor is not read.
 *   mode NPCD_SAMPLER_HOLD (no mask): exactly as in npcd_sampler_step; its hist pointer is not used and may be NULL.
 *   mask given (keep_coords / keep_feats, bytes [B, n_points]): as in npcd_sampler_step_keep -- x_t, eps, noise and known must all be
 *        given, `mode` is ignored, n_points must divide per_sample; kept points take h1[t] known + h2[t] noise, selected and not
 *        blended; hist and x0_out receive `known` there; nothing at a free point reads `known`.  n_points is read only with a mask.
 * Both tensors go in ONE launch on the grid rule of npcd_sampler_step; 16 bytes per lane under the alignment conditions of
 * npcd_sampler_step / npcd_sampler_step_keep with hist 16-byte aligned too, otherwise one element per lane; no atomics: the same bits
 * on every run from the same history.  NPCD_ERR_ARG / NPCD_ERR_UNSUPPORTED as for those two, and NPCD_ERR_ARG for a missing hist of a
 * tensor that is not in hold mode; all before any launch. */
int npcd_sampler_step_multistep(const NpcdSamplerTensor* coords, const NpcdSamplerTensor* feats, float* hist_coords, float* hist_feats,
                                const uint8_t* keep_coords, const uint8_t* keep_feats, int64_t n_points, const int64_t* t,
                                const float* table, int T, int B, void* stream);

/* Forward process and training loss of the DDPM, fused (reference gaussian_diffusion.py:68-76 q_sample, :199-230 p_losses):
 *   npcd_q_sample    : x_t = tab_sqrt_acp[t_b] * x_0 + tab_sqrt_1macp[t_b] * noise, fp32 [B, per_sample], t int64 [B]; the products
 *                      and the sum are rounded separately like the reference's eager ops (bit-identical to them)
 *   npcd_eps_mse_fwd : loss[0] = mean((noise - eps)^2 / 2) over numel elements (eps fp32 or bf16), optional pointwise output
 *                      (fp32 [numel] or NULL); part: fp32 scratch of npcd_eps_mse_blocks() elements; fixed-order sums
 *   npcd_eps_mse_bwd : grad = -(noise - eps) / numel * upstream_dev[0]   (grad has the dtype of eps) */
int npcd_q_sample(const float* x0, const float* noise, const int64_t* t, const float* tab_sqrt_acp, const float* tab_sqrt_1macp,
                  float* x_t, int B, int64_t per_sample, void* stream);
int npcd_eps_mse_blocks(void);
int npcd_eps_mse_fwd(const float* noise, const void* eps, int eps_dtype, int64_t numel, float* pointwise, float* part, float* loss,
                     void* stream);
int npcd_eps_mse_bwd(const float* noise, const void* eps, int eps_dtype, int64_t numel, const float* upstream_dev, void* grad,
                     void* stream);

/* ray march on the compact layout of npcd_grid_query_compact (same math as npcd_ray_march).  `capacity` = rows allocated in
 * sigma / rgb / pts: when the compact lists overflowed (counter[1] != 0) a ray whose rows lie past it is marched as empty --
 * the caller discards that result and retries with larger lists, nothing is read out of bounds meanwhile. */
int npcd_ray_march_compact(const float* sigma, const float* rgb, const uint64_t* ray_bits, const float* pts,
                           const int32_t* ray_base, const float* rays_o, const float* rays_d, const float* t1,
                           int Nr, int M, int capacity, int white_back, float* mask, float* depth, float* channels,
                           float* depth_ws, void* stream);

/* Fused render (ABI 9): two launches per view fewer, the same bits (Renderer.forward, renderer.py:202-268, for every pixel of
 * `views` views per example; ray_sampler.py:10-49 + renderer.py:36-47 + aggregator.py:63-73 + renderer.py:120-185).
 *   npcd_render_rays_query     = npcd_ray_gen + npcd_grid_query_compact_ordered in one query launch: the query kernel computes its ray
 *       from extr [B * views, 4, 4] (world2cam) / intr [B * views, 3, 3] and writes rays_o / rays_d [B, R, 3], t0 / t1 [B, R]
 *       (R = views * res^2) for the later stages.  t0 / t1 of a ray that misses the cube keep the raw -1 / -2; lim_part
 *       [npcd_render_lim_words(B, R)] receives per-group (min start, max end) keys of the rays that hit.  Needs the ordered form
 *       (order_ws) and box >= the grid's range on every axis (a missing ray then has no sample inside the grid: nothing is lost by not
 *       sampling it between the global limits); NPCD_ERR_UNSUPPORTED otherwise -- the caller then uses the separate entry points.
 *   npcd_ray_march_compact_fused = npcd_ray_march_compact that ends a missing ray at the global end taken from lim_part (the
 *       renderer.py:40-43 fix-up): t0 [Nr] as written by the query, lim_part / lim_pairs = npcd_render_lim_words(B, R) / 2. */
int64_t npcd_render_lim_words(int B, int R);
int npcd_render_rays_query(const npcd_grid_params* grid, const void* workspace, const float* points, int B, int N, const float* extr,
                           const float* intr, int views, int res, float box, int S, int M, int k, float r, float* rays_o, float* rays_d,
                           float* t0, float* t1, int32_t* counter, int32_t capacity, int32_t* ray_base, int32_t* ray_nsel,
                           uint64_t* ray_bits, int32_t* nb_idx, float* pts, void* order_ws, uint32_t* lim_part, void* stream);
int npcd_ray_march_compact_fused(const float* sigma, const float* rgb, const uint64_t* ray_bits, const float* pts, const int32_t* ray_base,
                                 const float* rays_o, const float* rays_d, const float* t0, const float* t1, const uint32_t* lim_part,
                                 int lim_pairs, int Nr, int M, int capacity, int white_back, float* mask, float* depth,
                                 float* channels, float* depth_ws, void* stream);

/* ---- stage-1 training path: the data movement around the per-pair MLP (aggregators/mlp.py:36-125,
 * positional_encoder.py:16-20, aggregator.py:122-144).  Pairs (shading point, neighbour) are compact and ordered by point:
 * flat [Q] = global neighbour index, owner [Q] = shading-point index, off / cnt [P] = first pair and number of pairs of a point.
 *   npcd_pair_input_fwd : x0 [Q, F + 3 + 6 nf] = [feat[flat] | rel | sin / cos bands of rel], w [Q] = 1 / (|rel| + 1e-5),
 *                         rel = pts[owner] - kp_pos[flat]
 *   npcd_pair_input_bwd : dfeat [B*N, F] += dx0[:, :F] scattered by flat (float atomics; dfeat must be zeroed by the caller)
 *   npcd_pair_aggregate : backward == 0: dst = agg [P, C] = sum over a point's pairs of w / (sum w) * src[q]  (src = local [Q, C]);
 *                         backward != 0: dst = dlocal [Q, C] = w / (sum w) * src[p]                      (src = dagg [P, C]) */
int npcd_pair_input_fwd(const int64_t* flat, const int64_t* owner, const float* pts, const float* kp_pos, const float* kp_feat,
                        int feat_dim, int n_freqs, int64_t n_pairs, float* x0, float* w, void* stream);
int npcd_pair_input_bwd(const int64_t* flat, const float* dx0, int feat_dim, int n_cols, int64_t n_pairs, float* dfeat, void* stream);
/* LeakyReLU backward fused with the bias-gradient column partials (stage-1 MLPs, utils/model.py:22-36): dy = dz * (z > 0 ? 1 :
 * slope) with z the activation output, part [npcd_leaky_bwd_blocks(rows) + npcd_colsum_scratch_rows()][N] = column partials of
 * dy for npcd_colsum_finalize.  dtype NPCD_F32 or NPCD_BF16; N * element size a multiple of 16 bytes that divides 4096. */
int npcd_leaky_bwd_blocks(int64_t rows);
int npcd_leaky_bwd_colsum(const void* dz, const void* z, void* dy, float* part, int64_t rows, int N, float slope, int dtype,
                          void* stream);
int npcd_pair_aggregate(int backward, const float* src, const float* w, const int64_t* off, const int64_t* cnt, int channels,
                        int64_t n_points, float* dst, void* stream);

/* ---- stage-1 training path: the per-pair aggregator MLP itself (aggregators/mlp.py:36-100; utils/model.py:22-36; pointnerf.py:
 * 174-179: Linear(F+63,256) + 3 x Linear(256,256), LeakyReLU(0.01) after each) on the matrix cores, forward AND backward, bf16
 * operands with fp32 accumulation (csrc/pairs_mlp.hip).  Pairs as above: row q of every [Q, .] array, ordered by point.
 *   npcd_pair_mlp_pack : fp32 DEVICE weights W_l [256, in_l] (in_0 = F + 63) / biases b_l [256], l = 0..3  ->  wpack (device,
 *                        npcd_pair_mlp_wpack_bytes()): bf16 fragment order of W_l (forward) and W_l^T (data gradient) + fp32 biases
 *   npcd_pair_mlp_fwd  : nb_idx [P,k] int64 (-1 pad, valid first), pts [P,3], kp_pos [B*N,3], kp_feat [B*N,F] fp32, off [P] int64
 *                        -> G [P,256] fp32 = inverse-distance weighted mean over a point's pairs of the 4th layer's output
 *                        (aggregators/mlp.py:102-125; the network's 5th, linear layer is applied by the caller on points);
 *                        saved for the backward: x0 [Q, F+64] bf16, acts [4][Q][256] bf16, wn [Q] fp32 (normalised weights)
 *   npcd_pair_mlp_bwd  : dG [P,256] fp32, owner [Q] int64 -> dfeat [Q,F] fp32 (gradient w.r.t. the gathered feature rows, to be
 *                        scattered with npcd_pair_input_bwd), dW[l] [256, in_l] fp32, db[l] [256] fp32 (overwritten; slabs summed
 *                        in a fixed order: bitwise reproducible).  dact: 2 x [Q,256] bf16 scratch; part: fp32 scratch of
 *                        npcd_pair_mlp_bwd_workspace_floats() elements.  F in {32, 128}.
 * `precision` (ABI 8) of every entry point:
 *   NPCD_PAIR_MLP_BF16 (0): bf16 operands, fp32 accumulation -- narrower than the reference's fp32 (train_pointnerf.py has no autocast);
 *   NPCD_PAIR_MLP_X2   (1): fp32-class -- every operand (weights, activations, gradients) as two bf16 halves hi + lo, every product
 *                        as three matrix instructions hi*hi + hi*lo + lo*hi accumulated in fp32: ~1e-5 relative per product, fp32's
 *                        exponent range.  All 16-bit arrays then hold TWO planes (hi, then lo): x0 [2][Q][F+64], acts [4][2][Q][256],
 *                        dact 2 x [2][Q][256]; wpack twice the matrices.  Same calls, same outputs (G, dfeat, dW, db: fp32).
 * Forward only (rendering with fp32-class shading): x0 = acts = wn = NULL -- nothing is saved. */
#define NPCD_PAIR_MLP_BF16 0
#define NPCD_PAIR_MLP_X2 1
int64_t npcd_pair_mlp_wpack_bytes(int feat_dim, int precision);
int npcd_pair_mlp_pack(const float* const* weights_dev, const float* const* biases_dev, int feat_dim, int precision, void* wpack_dev,
                       void* stream);
int npcd_pair_mlp_fwd(const void* wpack, int feat_dim, int precision, const int64_t* nb_idx, const float* pts, const float* kp_pos,
                      const float* kp_feat, const int64_t* off, int64_t n_points, int k, int64_t n_pairs, void* x0, void* acts,
                      float* wn, float* G, void* stream);
int npcd_pair_mlp_bwd_slabs(int64_t n_pairs, int precision);
int64_t npcd_pair_mlp_bwd_workspace_floats(int feat_dim, int64_t n_pairs, int precision);
int npcd_pair_mlp_bwd(const void* wpack, int feat_dim, int precision, const float* dG, const int64_t* owner, const float* wn,
                      const void* x0, const void* acts, int64_t n_pairs, void* dact, float* dfeat, float* part, float* const* dW,
                      float* const* db, void* stream);

/* ---- fp32-class forward of the denoiser's Linear layers (sampling in the reference's numerics class, diffusion_model.py:108-133;
 * transformer.py:67,107-115,118-137): x W^T on fp32 operands as ONE bf16 library GEMM over the three cross products of split operands,
 * [xh | xl | xh] [Wh | Wh | Wl]^T (x = xh + xl, bf16 halves; fp32 accumulation and output): 3e-6 relative, 2.3-3.5 x the fp32 GEMM's rate.
 * npcd_split3_bf16: the activation side in one pass: y = x [rows, K] fp32 (+ bias [K]) (-> exact-erf GELU if gelu != 0)  ->
 * out [rows, 3 K] bf16 = [hi(y) | lo(y) | hi(y)].  K % 8 == 0, 16-byte aligned pointers.  (ABI 8) */
int npcd_split3_bf16(const float* x, const float* bias, void* out, int64_t rows, int K, int gelu, void* stream);
/* The same hand-over behind a LayerNorm (transformer.py:169-172: x = x + attn(ln_1(x)); x = x + mlp(ln_2(x))), one pass:
 * xnew = x (+ o + bias, written when o is given);  out [rows, 3 W] = [hi | lo | hi] of LayerNorm(xnew) * gamma + beta (fp32 statistics, biased
 * variance).  o / bias / xnew: all three or none.  W in {256, 512, 768, 1024, 2048, 4096}.  (ABI 8) */
int npcd_add_ln_split3_bf16(const float* x, const float* o, const float* bias, const float* gamma, const float* beta, float* xnew,
                            void* out, int64_t rows, int W, float eps, void* stream);

/* ---- fp32-class TRAINING of the denoiser's residual blocks (DiffusionTrainer(dtype="fp32_class")): every forward, data-gradient and
 * weight-gradient product of a block as bf16 GEMMs over the three cross products hi*hi + lo*hi + hi*lo of split operands, fp32
 * accumulation; LayerNorm, GELU, attention and every column sum in fp32.  All sums in a fixed order, no atomics.
 * npcd_add_ln_split3_stats_bf16: npcd_add_ln_split3_bf16 that also writes the row statistics mean / rstd [rows] fp32 (the LayerNorm
 *   backward reads them).
 * npcd_split_weights_bf16: up to NPCD_SPLIT_WEIGHTS_MAX fp32 weights W [N, K] (the four Linear layers of a block) in one launch, each
 *   to both split layouts: fwd [N, 3 K] = [Wh | Wh | Wl] (the forward product's operand) and dgrad [3 N, K] = [Wh ; Wh ; Wl] (the data
 *   gradient's: [dyh | dyl | dyh] [3 N, K] = dyh Wh + dyl Wh + dyh Wl).  K % 8 == 0, 16-byte aligned pointers.
 * npcd_ln_bwd_split3_bf16: the LayerNorm backward of npcd_ln_bwd_dt with an fp32 dy and, in place of the 16-bit dxb, the split
 *   dx3 [T, 3 W] = [hi | lo | hi] of dx (may be NULL); dx and the column partials are computed exactly as there.
 * npcd_split3_colsum_bf16: v = a [T, N] fp32, or with gelu != 0 v = a * gelu_erf'(h + bias) (the GELU backward: a = dg, h = the c_fc
 *   output without its bias) -> out [T, 3 N] = [hi | lo | hi] of v, part [npcd_colsum_blocks(T)][N] fp32 column partials of v, finished
 *   by npcd_colsum_finalize.  N % 8 == 0, 16-byte aligned pointers. */
#define NPCD_SPLIT_WEIGHTS_MAX 8
typedef struct NpcdSplitWeight {
    const float* w; /* [N, K] fp32 */
    void* fwd;      /* [N, 3 K] bf16 */
    void* dgrad;    /* [3 N, K] bf16 */
    int N, K;
} NpcdSplitWeight;
int npcd_add_ln_split3_stats_bf16(const float* x, const float* o, const float* bias, const float* gamma, const float* beta, float* xnew,
                                  void* out, float* mean, float* rstd, int64_t rows, int W, float eps, void* stream);
int npcd_split_weights_bf16(const NpcdSplitWeight* desc, int count, void* stream);
int npcd_ln_bwd_split3_bf16(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                            const float* dres, float* dx, void* dx3, float* part_gamma, float* part_beta, float* part_col, int T, int W,
                            void* stream);
int npcd_split3_colsum_bf16(const float* a, const float* h, const float* bias, void* out, float* part, int T, int N, int gelu,
                            void* stream);

/* ---- stage-1 regularisers (csrc/stage1_losses.hip): the TV loss over each point's neighbour list (neural_point_cloud_tv_loss.py:29-83)
 * and the KL loss of the variational feature embedding (neural_point_cloud_kl_loss.py:29-44), one launch each way, no host wait.
 *   tv_i = weight_tv * sum_{j in list(i)} (1 / (|p_j - p_i| + 1e-5)) * sum_f |feat_j - feat_i|
 *   kl_i = weight_kl * (-0.5) * sum_f (1 + log_var - mean^2 - exp(log_var));     totals = means over B N
 * coords [B, N, 3] contiguous.  nb: int32 GLOBAL indices b N + j, -1 padded, row (b N + i) at nb + (b N + i) * nb_ld, k entries -- slot 0
 * of the dense query result [B, N, M, k] is read in place with nb_ld = M k.  LIST RULE: an entry is skipped when it is negative, when it
 * is the point itself (the reference drops self beside another neighbour and a lost point keeps itself: a self pair adds exactly 0 to
 * value and gradient), or when it lies outside [b N, (b + 1) N) (the query never returns one; a hand-made or stale list cannot read out
 * of bounds).  feats / mean / log_var: rows of F floats at row strides feats_ld / kl_ld / kl_ld.  nb == NULL leaves the TV term out,
 * mean == NULL the KL term (their outputs are then not touched); at least one is given.
 * Forward: tv_pointwise / kl_pointwise [B, N], tv_total / kl_total one float each; workspace: npcd_stage1_reg_workspace_floats(B)
 * floats, uninitialised (per-cloud partial sums; a one-wave second launch adds them in ascending cloud order).
 * Backward: the upstream gradient of point (b, i) is g_*_total[0] / (B N) + g_*_pointwise[b N + i]; each of the four may be NULL (= 0).
 * dfeats / dmean / dlog_var [B, N, F] contiguous, fully written.  The part of dfeats that comes from the lists naming a point is
 * gathered through a reverse table in ascending owner index: no float atomics, the same bits from run to run.  Coordinates get no
 * gradient (detached in the reference).
 * Supported: dtype NPCD_F32, N <= 4096, k N <= 32768, F <= 128; anything else is NPCD_ERR_UNSUPPORTED before any launch. */
int64_t npcd_stage1_reg_workspace_floats(int B);
int npcd_stage1_reg_fwd(const float* coords, const int32_t* nb, int64_t nb_ld, const float* feats, int64_t feats_ld, const float* mean,
                        const float* log_var, int64_t kl_ld, int B, int N, int k, int F, float weight_tv, float weight_kl, int dtype,
                        float* tv_pointwise, float* tv_total, float* kl_pointwise, float* kl_total, float* workspace, void* stream);
int npcd_stage1_reg_bwd(const float* coords, const int32_t* nb, int64_t nb_ld, const float* feats, int64_t feats_ld, const float* mean,
                        const float* log_var, int64_t kl_ld, int B, int N, int k, int F, float weight_tv, float weight_kl, int dtype,
                        const float* g_tv_total, const float* g_tv_pointwise, const float* g_kl_total, const float* g_kl_pointwise,
                        float* dfeats, float* dmean, float* dlog_var, void* stream);

/* ---- farthest point sampling (csrc/fps.hip): the operator of pytorch3d.ops.sample_farthest_points, which the
 * reference's dataset uses to cut a raw surface cloud down to num_points points (npcd/data/srn.py:179-188).
 * points [N, P, 3] fp32 contiguous.  lengths / ks / start: int32 [N] on the device, each may be NULL: valid points per cloud (P),
 * picks per cloud (Kmax), index of the first pick (0).  Cloud i makes min(ks[i], lengths[i], Kmax) picks: the start index, then again
 * and again the valid point whose squared distance to the nearest earlier pick, ((dx dx + dy dy) + dz dz) in fp32 without
 * contraction, is largest -- the LOWEST index among equals.  idx_out [N, Kmax] int64, pts_out [N, Kmax, 3] fp32 (bit copies of the
 * picked rows); the slots after a cloud's picks hold -1 and 0.0.  Both are fully written.  Integer-exact and the same on every run.
 * lengths are clamped to [0, P] and start to [0, length) on the device, so that no value read there reaches outside the cloud;
 * non-finite coordinates are not checked for (the result is then unspecified, never out of bounds).
 * One workgroup per cloud: up to npcd_fps_resident_points() points the cloud lives in registers, up to npcd_fps_max_points() it is
 * streamed from L2 at every pick.  NPCD_ERR_UNSUPPORTED for P above that, and for N, P or Kmax <= 0, before any pointer is looked at. */
int npcd_fps_resident_points(void);
int npcd_fps_max_points(void);
int npcd_fps(const float* points, const int32_t* lengths, const int32_t* ks, const int32_t* start, int64_t* idx_out, float* pts_out,
             int N, int P, int Kmax, void* stream);

/* ---- all-pairs directed Chamfer matrix (csrc/chamfer.hip): the distance under the shape metrics MMD-CD / COV-CD /
 * 1-NNA-CD of npcd/eval/shapes.py.  x [M, P, 3], y [N, Q, 3] fp32 contiguous; x_len / y_len: int32 [M] / [N] on the device, valid
 * points per cloud, either may be NULL (P / Q).  out [M, N] fp32, fully written:
 *   out[i, j] = ( sum_{p < Lx_i} min_{q < Ly_j} d(x_ip, y_jq) ) / Lx_i,   d(a, b) = ((dx dx + dy dy) + dz dz), dx = a.x - b.x ...
 * in fp32 without contraction.  min is exact, so every per-point minimum is the bits of that expression; the sum over p has one fixed
 * order (no float atomics: the same bits on every run) and, with the division, is all that rounds.  The norm-expansion form is not
 * used.  Lengths are clamped to [1, P] and [1, Q] on the device; rows at or after a cloud's length are never looked at for the result
 * and no read leaves the arrays whatever the lengths hold; non-finite coordinates are not checked for (the result is then
 * unspecified, never out of bounds).  x and y are only read and may be the same pointer.  No workspace, no scratch.
 * NPCD_ERR_UNSUPPORTED for M, N, P or Q <= 0, for P or Q above npcd_chamfer_max_points() (4,096) and for M or N above 16,384, before
 * any pointer is looked at; NPCD_ERR_ARG for a NULL x, y or out. */
int npcd_chamfer_max_points(void);
int npcd_chamfer_directed(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, float* out, int M, int P, int N,
                          int Q, void* stream);

/* ---- all-pairs directed approximate earth mover's distance (csrc/emd.hip): the second distance under the shape
 * metrics of npcd/eval/shapes.py (MMD-EMD / COV-EMD / 1-NNA-EMD).  Arguments, null lengths and the clamping of lengths as for
 * npcd_chamfer_directed.  out [M, N] fp32, fully written: the cost of the approximate matching of Fan et al. between the valid rows
 * of x_i and y_j -- ten levels exp(level d), level = -4^7 ... -4^0, -4^-1, 0, three passes each, d as above -- divided by
 * T = max(Lx, Ly); directed, out(x, y) != out(y, x) in general.  All fp32; every sum has one fixed order and there are no float
 * atomics: the same bits on every run.  The match matrix is never stored.  No read leaves the arrays whatever the lengths hold;
 * non-finite coordinates are not checked for.  x and y are only read and may be the same pointer.  No workspace, no scratch.
 * NPCD_ERR_UNSUPPORTED for M, N, P or Q <= 0, for P or Q above npcd_emd_max_points() (2,048) and for M or N above 16,384, before any
 * pointer is looked at; NPCD_ERR_ARG for a NULL x, y or out. */
int npcd_emd_max_points(void);
int npcd_emd_directed(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, float* out, int M, int P, int N, int Q,
                      void* stream);

/* ---- occupancy grid of point clouds (csrc/occupancy.hip): the operator under the Jensen-Shannon divergence and the
 * occupancy entropy of npcd/eval/shapes.py.  points [n, P, 3] fp32 contiguous; lengths int32 [n] on the device or NULL (P), clamped
 * to [1, P].  lattice [R] fp32: the cell centres along an axis, ascending, the same on the three axes; cell (i, j, k) has the flat
 * index (i R + j) R + k.  The valid cells are data: k_lo / k_hi [R * R] bytes, per column (i, j) the inclusive range of valid k,
 * k_lo > k_hi an empty column (k_hi is read as min(k_hi, R - 1)).  Every point with finite coordinates in a row before its cloud's
 * length goes to the valid cell whose centre is nearest (squared Euclidean distance, fp32 on direct differences; among equal
 * distances the lowest index) and is counted:
 *   counts [R^3] int32 += points in the cell;   clouds [R^3] int32 += clouds with at least one point in the cell;
 *   cells [n, P] int32 or NULL, fully written: the point's cell, -1 for a row at or after the length and for a non-finite point.
 * counts and clouds are accumulated into: the caller zeroes them, and may feed a set in several calls.  Integer atomics only: the
 * same bits on every run.  A mask without a valid cell counts nothing.  No read leaves the arrays whatever the lengths or the mask
 * hold.  A cloud is never split over workgroups: npcd_occupancy_clouds_per_workgroup(n, P, R) clouds go to each.
 * NPCD_ERR_UNSUPPORTED for n or P <= 0, n P >= 2^31 and R outside [2, npcd_occupancy_max_resolution()] (32), before any pointer is
 * looked at; NPCD_ERR_ARG for a NULL pointer other than lengths and cells.  Nothing is launched in either case. */
int npcd_occupancy_max_resolution(void);
int npcd_occupancy_clouds_per_workgroup(int n, int P, int R);
int npcd_occupancy_grid(const float* points, const int32_t* lengths, const float* lattice, const uint8_t* k_lo, const uint8_t* k_hi,
                        int32_t* counts, int32_t* clouds, int32_t* cells, int n, int P, int R, void* stream);

/* ---- image metrics of rendered views (csrc/ssim.hip): the structural similarity index (SSIM) and the mean squared
 * error under npcd.eval.ssim / psnr and the ssim= switch of evaluate_pointnerf.  pred, target: fp32 images of V views, C channels,
 * H x W pixels, element (v, c, i, j) at v sv + c sc + i sh + j sw of its own four ELEMENT strides -- [V, C, H, W] and the renderer's
 * pixel-interleaved [V, H, W, C] are both read in place; only read, and may be the same pointer.  taps [w] float64 on the device: a
 * separable window, w odd in [3, 15], the taps summing to 1.  With x = pred, y = target read as float64, at each of the
 * (H - w + 1) (W - w + 1) valid positions, where the window lies inside the image,
 *   ux, uy, uxx, uyy, uxy = window means of x, y, x x, y y, x y with weights taps[i] taps[j];
 *   vx = n (uxx - ux ux), vy = n (uyy - uy uy), vxy = n (uxy - ux uy);
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux ux + uy uy + C1)(vx + vy + C2)),  C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;
 * all float64, evaluated as written.  Outputs, float64, fully written:
 *   ssim [V, C] = mean of S over the valid positions;   mse [V] = mean of (x - y)^2 over all C H W pixels of the view;
 *   map [V, C, H - w + 1, W - w + 1] or NULL = S.
 * n = w^2 / (w^2 - 1) with uniform taps 1 / w is skimage.metrics.structural_similarity at its defaults (sample covariance), n = 1 with
 * Gaussian taps the setting of Wang et al.  Identical images give ssim = 1 and mse = 0 exactly.  A non-finite pixel makes the mse of
 * its view, the ssim of its (view, channel) and S at every window that holds it NaN, and touches no other view.
 * workspace: npcd_image_metrics_workspace_bytes(V, C, H, W, w) bytes, 8-byte aligned, contents irrelevant before and after: two
 * partial sums per tile of npcd_image_metrics_tile() = (rows, cols) valid positions of one (view, channel), added by a second small
 * launch in a fixed order.  No float atomics: the same bits on every run, and a view's numbers do not depend on the other views of the
 * call.  No scratch.
 * NPCD_ERR_UNSUPPORTED (the workspace query returns it too) for V, C, H or W <= 0, H or W < w, w even or outside [3, 15] and
 * V C H W >= 2^31, before any pointer is looked at; NPCD_ERR_ARG for a NULL pointer other than map and for data_range or n not positive
 * and finite.  Nothing is launched in either case.  rows_host / cols_host are host pointers. */
int npcd_image_metrics_tile(int* rows_host, int* cols_host);
int64_t npcd_image_metrics_workspace_bytes(int V, int C, int H, int W, int w);
int npcd_image_metrics(const float* pred, const float* target, int V, int C, int H, int W, int64_t pred_sv, int64_t pred_sc,
                       int64_t pred_sh, int64_t pred_sw, int64_t target_sv, int64_t target_sc, int64_t target_sh, int64_t target_sw,
                       const double* taps, int w, double n, double data_range, double* workspace, double* mse, double* ssim, double* map,
                       void* stream);

/* ---- feature statistics: the moments of the Frechet distance and the subset sums of the kernel inception distance --------------------
 * (csrc/feature_stats.hip).  Features are rows of [N, D] matrices on the device, dtype NPCD_F32 or NPCD_F64, a row
 * stride in elements (>= D) and unit column stride, only read.  All arithmetic is float64 on the float64 matrix instruction; every
 * accumulator element is owned by one lane of one workgroup: no float atomics, no fence, the same bits on every run.
 *
 * npcd_moments_update: over the rows [r0, r1) of x, with s = shift [D] (float64, NULL = 0),
 *   sum[j] += SUM_r (x_rj - s_j);    gram[i][j] += SUM_r (x_ri - s_i)(x_rj - s_j)   where tile(j) >= tile(i),
 * tile(c) = c / T with T of npcd_moments_tile; entries of gram [D, D] in tiles below the diagonal are not touched.  One launch;
 * r1 == r0 launches nothing.  sum [D] and gram are float64 and must hold the totals so far (zeros at first).
 * npcd_moments_finish: mean[j] = s_j + sum[j] / n;  cov[i][j] = cov[j][i] = (gram[i][j] - n m_i m_j) / (n - 1), m = sum / n, from the
 * upper tiles of gram: the full symmetric [D, D], both halves written from one computed value.  n is the number of rows summed.
 *
 * npcd_kid_subsets: idx_f, idx_r int32 [S, m] on the device, entries in [0, Nf) and [0, Nr).  With x_i = fake[idx_f[s, i]],
 * y_j = real[idx_r[s, j]], k(a, b) = t t t, t = (a . b) / D + 1,
 *   out[s] = (SUM_{i != j} k(x_i, x_j),  SUM_{i != j} k(y_i, y_j),  SUM_{i, j} k(x_i, y_j)),   out float64 [S, 3], fully written.
 * workspace: npcd_kid_workspace_bytes(S, m) bytes, 8-byte aligned, contents irrelevant before and after: one partial sum per tile of
 * npcd_kid_tile = T x T pairs, S (t (t + 1) + t t) of them with t = ceil(m / T) (only the tiles on or above the diagonal of the two
 * symmetric matrices are computed), added by a second small launch in a fixed order.
 *
 * NPCD_ERR_UNSUPPORTED for D < 1 or D > npcd_moments_max_features() (4,096), a dtype other than the two, n < 2, m < 2, m > 2^20, S < 1
 * and S times the tiles of a subset >= 2^31 (the workspace query returns it too), before any pointer is looked at; NPCD_ERR_ARG for a
 * NULL pointer other than shift, r0 < 0, r1 < r0, a row stride below D, Nf or Nr < 1.  Nothing is launched in either case.  tile_host
 * is a host pointer. */
int npcd_moments_tile(int* tile_host);
int npcd_moments_max_features(void);
int npcd_moments_update(const void* x, int dtype, int64_t ld, int64_t r0, int64_t r1, int D, const double* shift, double* sum, double* gram,
                        void* stream);
int npcd_moments_finish(const double* sum, const double* gram, const double* shift, int D, int64_t n, double* mean, double* cov,
                        void* stream);
int npcd_kid_tile(int* tile_host);
int64_t npcd_kid_workspace_bytes(int S, int m);
int npcd_kid_subsets(const void* fake, const void* real, int dtype, int Nf, int Nr, int D, int64_t ldf, int64_t ldr, const int32_t* idx_f,
                     const int32_t* idx_r, int S, int m, double* workspace, double* out, void* stream);

/* ---- feature k-NN: the radii and ball counts behind precision / recall and density / coverage -------------------------------------------
 * (csrc/feature_manifold.hip).  x [n, D] and y [m, D] are features on the device, dtype NPCD_F32 or NPCD_F64 (one for
 * both), a row stride in elements (>= D) and unit column stride, only read; y may be x.  All arithmetic is float64 on the float64 matrix
 * instruction:
 *   d2_ij = max((nx_i + ny_j) - 2 g_ij, +0),   g_ij = x_i . y_j,   nx_i = x_i . x_i,   ny_j = y_j . y_j,
 * evaluated as written.  Columns j >= m do not exist; with exclude_self = 1 the pair j == i does not exist either (by index, not by
 * value).  The distances are streamed tile by tile and never stored.
 *
 * npcd_feature_knn: out [n, k] float64 = the k smallest d2_ij of every row i, ascending, equal values kept (a multiset), fully
 *   written.  1 <= k <= npcd_feature_knn_max_k() (8).
 * npcd_feature_ball_counts: rho_y float64 [m];  cnt[i] = #{j : d2_ij < rho_y[j]} (int32 [n], strict),  near[i] = min_j d2_ij
 *   (float64 [n]), fully written.
 * splits: workgroups per block of 64 rows of x, each taking a contiguous range of the 64-row tiles of y; 0 lets the library choose
 *   from n and m, a value above the number of tiles (or above 256) is lowered to it.  The results are the same bits for every value
 *   and on every run: no atomics, no fence; the partial results of the splits are merged by a second small launch in a fixed order.
 * workspace: npcd_feature_rows_workspace_bytes(n, m, k, splits) bytes (k = 0: for the ball counts), 8-byte aligned, contents
 *   irrelevant before and after: 8 (n + m) for the norms, plus 8 S n k (k-NN) or 16 S n (ball counts) for the partial results when
 *   the S splits in effect are more than one.
 *
 * NPCD_ERR_UNSUPPORTED for D < 1 or D > 4,096, a dtype other than the two, k out of range, m - exclude_self < k, n < 1, m < 1, n or
 * m > 2^24, splits < 0 and exclude_self other than 0 / 1 (the workspace query returns it too), before any pointer is looked at;
 * NPCD_ERR_ARG for a NULL pointer or a row stride below D.  Nothing is launched in either case. */
int npcd_feature_knn_max_k(void);
int64_t npcd_feature_rows_workspace_bytes(int n, int m, int k, int splits);
int npcd_feature_knn(const void* x, const void* y, int dtype, int n, int m, int D, int64_t ldx, int64_t ldy, int exclude_self, int k,
                     int splits, double* workspace, double* out, void* stream);
int npcd_feature_ball_counts(const void* x, const void* y, int dtype, int n, int m, int D, int64_t ldx, int64_t ldy, const double* rho_y,
                             int splits, double* workspace, int32_t* cnt, double* near, void* stream);

/* ---- isosurface of a density volume (csrc/isosurface.hip): marching tetrahedra on the Kuhn triangulation of the
 * lattice, the operator under npcd/eval/mesh.py.  vol [B, gz, gy, gx] fp32 contiguous, x fastest; node (x, y, z) has the index
 * (z gy + y) gx + x and lies at origin + spacing * (x, y, z) (origin_host / spacing_host: three floats each, x y z).  A node is
 * inside iff f > level.  The surface is a function of the volume alone -- which edges carry a vertex, the vertex on an edge
 * (t = (level - f_lo) / (f_hi - f_lo), fp32 as written), the order of vertices and triangles, the winding (inside -> outside) and
 * the canonical form of a triangle are stated in DESIGN.md 5.13 and restated by npcd.eval.mesh.marching_tetrahedra_reference.
 *   npcd_isosurface_count: counts [B, 2] int64 = (vertices, triangles) of every volume, and in ws (npcd_isosurface_ws_bytes, 8-byte
 *       aligned) what the second call needs: per node one word (bits 0-6 the crossed edge types, bit 7 "inside", bits 8.. the vertices
 *       of the node's 1,024-node strip before it), per strip the exclusive vertex (int32) and triangle (int64) bases.  Two launches.
 *   npcd_isosurface_emit:  vertices [sum V, 3] fp32 and faces [sum F, 3] int32 with indices local to their volume; volume b writes at
 *       rows vert_offsets[b] / face_offsets[b] (int64 [B], the exclusive sums of counts).  What it writes follows from ws alone: exactly
 *       counts[b] rows, whatever vol and level hold at this call.  One launch.
 * The caller reads counts between the two calls to size the outputs.  Exclusive sums in a fixed order, no atomics: the same bits on
 * every run.  A volume without a crossing is valid: (0, 0), and emit need not be called when nothing is to be written.
 * NPCD_ERR_ARG for B < 1, an axis below 2 nodes, a NULL pointer or a misaligned ws; NPCD_ERR_UNSUPPORTED for 7 gz gy gx >= 2^31 (the
 * workspace query returns both too).  Nothing is launched in either case. */
int64_t npcd_isosurface_ws_bytes(int B, int gz, int gy, int gx);
int npcd_isosurface_count(const float* vol, int B, int gz, int gy, int gx, float level, void* ws, int64_t* counts, void* stream);
int npcd_isosurface_emit(const float* vol, int B, int gz, int gy, int gx, float level, const float* origin_host, const float* spacing_host,
                         const void* ws, const int64_t* vert_offsets, const int64_t* face_offsets, float* vertices, int32_t* faces,
                         void* stream);

/* ---- finishing a mesh (added within ABI 10): connected components of the volume, to drop floaters before the
 * isosurface is taken, and vertex normals.  vol as above; the specification is restated by connected_components_reference and
 * vertex_normals_reference of npcd/eval/mesh.py, and the kernels are held to them bit for bit.
 *   npcd_components_label (csrc/components.hip): two inside nodes (f > level, NaN outside) are adjacent iff they are the two ends of
 *       one of the isosurface's seven edge types -- 14 neighbours a node.  labels [B, gz, gy, gx] int32 = -1 outside, otherwise the
 *       smallest node index of the node's component, local to its volume; sizes, the same shape = the component's number of nodes at
 *       its root node, 0 elsewhere; both fully written.  ws: npcd_components_ws_bytes = 4 B gz gy gx bytes, contents irrelevant
 *       before and after.  A union-find in three launches (bricks of 16 x 8 x 8 nodes in LDS, the edges between bricks, the labels
 *       and sizes) on integer minima and additions only: the same bits on every run.  No host synchronisation, no allocation.
 *       NPCD_ERR_ARG for B < 1, an axis below 2 nodes, a NULL pointer or one that is not 4-byte aligned; NPCD_ERR_UNSUPPORTED for
 *       gz gy gx >= 2^31 (the workspace query returns both too).  Nothing is launched in either case.
 *   npcd_isosurface_normals (csrc/isosurface_normals.hip): normals [sum V, 3] fp32 in the rows npcd_isosurface_emit writes its
 *       vertices to, from the workspace npcd_isosurface_count(vol, ...) left (ws, vert_offsets, level and spacing_host as for emit).
 *       The vertex on the edge (lo, hi), t = (level - f_lo) / (f_hi - f_lo) from vol, gets n = (-g) / sqrt((gx gx + gy gy) + gz gz),
 *       g = g_lo + t (g_hi - g_lo), where the node gradients are those of `field` (which may be vol): (f[i + 1] - f[i - 1]) / (2 s) in
 *       the interior, (f[1] - f[0]) / (1 s) and (f[last] - f[last - 1]) / (1 s) at the borders, fp32 as written.  A normal with a
 *       component that is not finite is (+0, +0, +0).  One launch.  Refusals as for npcd_isosurface_emit. */
int64_t npcd_components_ws_bytes(int B, int gz, int gy, int gx);
int npcd_components_label(const float* vol, int B, int gz, int gy, int gx, float level, void* ws, int32_t* labels, int32_t* sizes,
                          void* stream);
int npcd_isosurface_normals(const float* vol, const float* field, int B, int gz, int gy, int gx, float level, const float* spacing_host,
                            const void* ws, const int64_t* vert_offsets, float* normals, void* stream);

/* ---- points on mesh surfaces, uniform by area (added within ABI 10; csrc/surface.hip, csrc/surface.h).  A batch of B
 * meshes is packed: vertices [V_total, 3] fp32 and faces [F_total, 3] int32 concatenated, a face's indices local to its mesh, and
 * vert_offsets / face_offsets [B + 1] int32 ON THE DEVICE (ascending, first 0, last the total; a member whose pair of offsets does
 * not ascend inside [0, total] counts as empty).  The specification is restated by face_weights_reference and
 * surface_sample_reference of npcd/eval/mesh.py, and the kernels are held to them bit for bit.
 *   npcd_surface_prepare: per face d = |e1 x e2| (fp32 as written; +0 where not finite or an index lies outside [0, V), through which
 *       nothing is read), per mesh d_max by an integer maximum on the bits, k = 31 - floor(log2 d_max), the integer weights
 *       w = floor(float64(d) 2^k) < 2^32, their inclusive sums inside every tile of 256 faces (kSurfTile of csrc/surface.h) and the
 *       inclusive sums of the tile totals; area [B] float64 = 0.5 float64(W) 2^-k, 0 for a mesh without faces or measure.  ws:
 *       npcd_surface_ws_bytes(B, F_total), 8-byte aligned; contents irrelevant before, the input of npcd_surface_sample after.  One
 *       4 B-byte memset and three launches; integer sums and maxima only: the same bits on every run.
 *   npcd_surface_sample: u [B, S, 3] fp32 -> points [B, S, 3]; faces_out [B, S] int32 or NULL (the face of every sample, local to its
 *       mesh); normals_mode 0: none (normals_out NULL), 1: the face's n / d (vertex_normals NULL), 2: the vertex_normals [V_total, 3]
 *       mixed with the sample's barycentric weights and normalised, (+0, +0, +0) where a component is not finite; normals_out [B, S, 3];
 *       attributes [V_total, C] fp32 mixed the same way into attributes_out [B, S, C], 1 <= C <= 16, or C = 0 and both NULL.
 *       k0 = clamp(floor(u0 2^24), 0, 2^24 - 1), r = floor(k0 W / 2^24) exactly, the face the smallest i whose inclusive sum exceeds
 *       r; s = sqrt(u1), b = (1 - s, s (1 - u2), s u2), every row (b0 x0 + b1 x1) + b2 x2.  A mesh with W = 0 gives face -1 and +0
 *       rows.  One launch; the tile sums of a mesh of up to 4,096 tiles (kSurfLdsTiles) are searched in LDS, those of a
 *       larger one in global memory.  vertices, faces and the offsets are those npcd_surface_prepare saw.
 * No host synchronisation, no allocation, no workgroup that waits on another.  NPCD_ERR_ARG for B < 1, S < 1, a negative total or C,
 * a NULL pointer (or one that the mode does not take), a misaligned ws or area; NPCD_ERR_UNSUPPORTED for V_total or F_total >= 2^31,
 * C > 16, B > 65,535 in npcd_surface_sample and B S max(3, C) >= 2^31 (the workspace query returns both too).  Nothing is launched in
 * either case. */
int64_t npcd_surface_ws_bytes(int B, int64_t F_total);
int npcd_surface_prepare(const float* vertices, const int32_t* faces, const int32_t* vert_offsets, const int32_t* face_offsets, int B,
                         int64_t V_total, int64_t F_total, void* ws, double* area, void* stream);
int npcd_surface_sample(const float* vertices, const int32_t* faces, const int32_t* vert_offsets, const int32_t* face_offsets, int B,
                        int64_t V_total, int64_t F_total, const void* ws, const float* u, int S, float* points, int32_t* faces_out,
                        int normals_mode, const float* vertex_normals, float* normals_out, const float* attributes, int C,
                        float* attributes_out, void* stream);

/* ---- vertex clustering of one mesh (added within ABI 10; csrc/simplify.hip, csrc/simplify.h).  vertices [V, 3] fp32,
 * faces [F, 3] int32, attributes [V, C] fp32 (0 <= C <= 16, NULL with C = 0) on the device; the grid on the HOST: origin_host [3] and
 * cell_host [3] float64 (finite, cell > 0), dims_host [3] int (each >= 1, the product at most 2^30).  The specification is restated
 * by simplify_reference of npcd/eval/mesh.py, and the kernels are held to it bit for bit.  The four calls of one mesh take the same
 * V, F, C and dims and one workspace of npcd_simplify_ws_bytes(V, F, C, dims_host) bytes, 8-byte aligned, contents irrelevant before.
 *   npcd_simplify_cluster: per vertex u = (float64(v) - origin) / cell, lost (-1) if not finite, c = clamp(floor(u), 0, dims - 1),
 *       key = (cz dims_y + cy) dims_x + cx, r = clamp(floor((u - c) 2^32), 0, 2^32 - 1); vertex_cluster [V] int32 = the rank of the
 *       vertex's key among the occupied cells; counts[0] (int64 [2] on the device) = V', the occupied cells; in ws the integer sums of
 *       r, of 1 and of the attributes q = rint(float64(a) 2^(30 - e)), e the exponent of the largest finite |a| of the call (a value
 *       that is not finite counts as 0).  One memset and four launches; V >= 1.
 *   npcd_simplify_faces: per face the clusters of its corners (in ws) and the sort keys of its sorted triple: key_hi NULL: one key
 *       a 2^42 + b 2^21 + c in key_lo [F] int64 (refused with NPCD_ERR_ARG when min(V, cells) > 2^21), else key_hi [F] = a and
 *       key_lo = b 2^32 + c; INT64_MAX in both for a face that goes: an index outside [0, V) (nothing is read through it), a lost
 *       corner, two corners in one cluster.  One launch; F >= 1.
 *   npcd_simplify_unique: order [F] int64 = the faces in a STABLE ascending order of those keys (by key_lo, then stably by key_hi).  A
 *       face stays if it is valid and the first of its run of equal sorted triples: the lowest input index.  counts[1] = F'.  An
 *       entry of order outside [0, F) is not followed.  One memset and three launches.
 *   npcd_simplify_emit: V_out = V' and F_out = F' as read from counts.  vertices_out [V', 3] fp32 = origin + cell (c + (float64(S) /
 *       float64(n)) 2^-32) in float64 as written; attributes_out [V', C] = fp32 of (float64(sum) / float64(n)) 2^(e - 30); faces_out
 *       [F', 3] the kept faces on the new vertices, corner order and input order kept, face_source [F'] int32 their input indices
 *       (both NULL with F_out = 0).  Two launches.  V_out in [1, min(V, cells)], F_out in [0, F].
 * Integer ORs, maxima and sums only: the same bits on every run.  No host synchronisation, no allocation, no workgroup that waits on
 * another.  NPCD_ERR_ARG for a negative size, V < 1 or F < 1 where stated, a dims entry below 1, an origin or cell that is not
 * finite or a cell <= 0, a NULL pointer (or one that the sizes do not take) or a misaligned one; NPCD_ERR_UNSUPPORTED for C > 16, V or
 * F >= 2^31 and more than 2^30 cells (the workspace query returns both too).  Nothing is launched in either case. */
int64_t npcd_simplify_ws_bytes(int64_t V, int64_t F, int C, const int* dims_host);
int npcd_simplify_cluster(const float* vertices, int64_t V, int64_t F, const float* attributes, int C, const double* origin_host,
                          const double* cell_host, const int* dims_host, void* ws, int32_t* vertex_cluster, int64_t* counts, void* stream);
int npcd_simplify_faces(const int32_t* faces, int64_t V, int64_t F, int C, const int* dims_host, const int32_t* vertex_cluster, void* ws,
                        int64_t* key_hi, int64_t* key_lo, void* stream);
int npcd_simplify_unique(const int64_t* order, int64_t V, int64_t F, int C, const int* dims_host, void* ws, int64_t* counts, void* stream);
int npcd_simplify_emit(int64_t V, int64_t F, int C, const double* origin_host, const double* cell_host, const int* dims_host,
                       const void* ws, int64_t V_out, int64_t F_out, float* vertices_out, float* attributes_out, int32_t* faces_out,
                       int32_t* face_source, void* stream);

/* ---- the edges of one mesh and Taubin smoothing on an integer lattice (added within ABI 10; csrc/smooth.hip,
 * csrc/smooth.h).  faces [F, 3] int32 and vertices [V, 3] fp32 on the device, 1 <= V < 2^31, 1 <= F < 2^28.  The specification is
 * restated by mesh_edges_reference and smooth_reference of npcd/eval/mesh.py, and the kernels are held to both bit for bit.
 *   npcd_mesh_edges_keys: keys [F, 6] int64.  A face is valid if its indices lie in [0, V) and differ pairwise; (i, j, k) gives the
 *       pairs i->j, j->k, k->i (forward), then j->i, k->j, i->k (backward).  The key of a->b is a 2^31 + b; what is written, and
 *       sorted, is key 2 + backward.  A face that is not valid gives six times INT64_MAX, and nothing is read through it.  One launch.
 *   npcd_mesh_edges_unique: sorted_keys [6F] int64 = those keys in ascending order.  counts (int64 [6] on the device) is zeroed, then
 *       counts[0] = D, the distinct keys (even), counts[1] = F_v, the valid faces; in ws (npcd_mesh_edges_ws_bytes(V, F) bytes, 8-byte
 *       aligned, contents irrelevant before) the ranks of the run heads.  One memset and two launches.
 *   npcd_mesh_edges_emit: D as read from counts[0], at least 2.  neighbours [D] int32 = the b of the distinct keys in order; row_start
 *       [V + 1] int32 = the distinct keys with a < v; edges [D / 2, 2] int32 = the distinct keys with a < b in order; edge_faces [D / 2]
 *       int32 = the faces that hold the edge (the length of its run), edge_forward [D / 2] int32 = those that traverse it as a->b;
 *       boundary_vertex [V] uint8 = 1 on an edge of one face; counts[2..5] = the used vertices (rows that are not empty), the edges
 *       of one face, of three or more, and of two that both traverse it the same way, summed per strip in ws and then by one workgroup:
 *       no atomics.  One memset and two launches.
 *   npcd_smooth_mesh: `iterations` (0 .. 1000) times a step with factor lam (0 < lam <= 1), then one with mu (-1 <= mu <= 0; mu = 0:
 *       no second step) on the adjacency (row_start, neighbours, D) of the calls above.  A = the largest finite |coordinate|, e =
 *       floor(log2 A), q = rint(float64(x) 2^(29 - e)); a vertex with a coordinate that is not finite is lost.  A vertex moves if it is
 *       not lost, has a neighbour that is not lost and neither fixed[v] nor boundary_vertex[v] (uint8 [V], either may be NULL) is set.
 *       A step: S the integer sum of q over the d neighbours that are not lost, q' = clamp(q + rint(f (float64(S) / float64(d) -
 *       float64(q))), -(2^31 - 1), 2^31 - 1), every vertex reading the old state.  vertices_out [V, 3] = fp32 of float64(q) 2^(e - 29)
 *       for a vertex that moves, the input bits for every other (for all with iterations = 0, D = 0 or A = 0).  ws:
 *       npcd_smooth_ws_bytes(V) bytes, 16-byte aligned.  One memset and 3 + steps launches; the step launches use no atomics.
 * Integer maxima and sums only: the same bits on every run.  No host synchronisation, no allocation, no workgroup that waits on
 * another.  NPCD_ERR_ARG for a negative size, V < 1 or F < 1, a D that is odd, below 2 or above 6F, iterations, lam or mu outside
 * their ranges, a NULL pointer that the call takes or a misaligned one; NPCD_ERR_UNSUPPORTED for V >= 2^31 or F >= 2^28 (the
 * workspace queries return both too).  Nothing is launched in either case. */
int64_t npcd_mesh_edges_ws_bytes(int64_t V, int64_t F);
int npcd_mesh_edges_keys(const int32_t* faces, int64_t V, int64_t F, int64_t* keys, void* stream);
int npcd_mesh_edges_unique(const int64_t* sorted_keys, int64_t V, int64_t F, void* ws, int64_t* counts, void* stream);
int npcd_mesh_edges_emit(const int64_t* sorted_keys, int64_t V, int64_t F, void* ws, int64_t D, int32_t* row_start,
                         int32_t* neighbours, int32_t* edges, int32_t* edge_faces, int32_t* edge_forward, uint8_t* boundary_vertex,
                         int64_t* counts, void* stream);
int64_t npcd_smooth_ws_bytes(int64_t V);
int npcd_smooth_mesh(const float* vertices, int64_t V, const int32_t* row_start, const int32_t* neighbours, int64_t D,
                     const uint8_t* boundary_vertex, const uint8_t* fixed, int iterations, double lam, double mu, void* ws,
                     float* vertices_out, void* stream);

/* ---- the closest point of one mesh to every query point (added within ABI 10; csrc/mesh_distance.hip,
 * csrc/mesh_distance.h).  points [S, 3], vertices [V, 3] fp32 and faces [F, 3] int32 on the device, V < 2^31, 1 <= F < 2^28,
 * 1 <= S < 2^31.  The specification is restated by point_mesh_distance_reference of npcd/eval/mesh.py, and the kernels are held to it
 * bit for bit.
 *   npcd_mesh_distance_boxes: ws (npcd_mesh_distance_ws_bytes(V, F) bytes, 16-byte aligned, contents irrelevant before) takes the
 *       corners of every face as three 16-byte words -- NaN for a face with an index outside [0, V), which is not followed -- and per
 *       tile of 256 consecutive faces the box of its finite corners.  One launch.
 *   npcd_mesh_distance_query: ws as the boxes call of the same (vertices, V, faces, F) left it.  Per point the lexicographic minimum of
 *       (dist2, face) over the faces with dist2 < +inf, dist2 the region form of Ericson's closest point on a triangle in fp32 as
 *       written: sqdist [S] fp32, face [S] int32, closest [S, 3] fp32; (+inf, -1, zeros) for a point that no face wins.  cull = 1
 *       skips a tile whose box lies farther from every point of a wave than the wave's best; cull = 0 evaluates every tile.  The
 *       outputs are the same bits.  evaluated (int64 on the device, may be NULL, not zeroed here) takes the (wave, tile) evaluations,
 *       one integer add per wave.  One launch.
 * No float atomics, no host synchronisation, no allocation, no workgroup that waits on another.  NPCD_ERR_UNSUPPORTED for V >= 2^31,
 * F >= 2^28 or S >= 2^31 (the workspace query returns it too); NPCD_ERR_ARG for a negative size, F < 1 or S < 1, a cull that is not 0
 * or 1, a NULL pointer that the call takes or a misaligned one.  Nothing is launched in either case. */
int64_t npcd_mesh_distance_ws_bytes(int64_t V, int64_t F);
int npcd_mesh_distance_boxes(const float* vertices, int64_t V, const int32_t* faces, int64_t F, void* ws, void* stream);
int npcd_mesh_distance_query(const float* points, int64_t S, const float* vertices, int64_t V, const int32_t* faces, int64_t F,
                             const void* ws, int cull, float* sqdist, int32_t* face, float* closest, int64_t* evaluated, void* stream);

/* ---- the first hit of every ray on one mesh (added within ABI 10; csrc/raycast.hip, csrc/raycast.h).  origins and
 * directions [R, 3], vertices [V, 3] fp32 and faces [F, 3] int32 on the device, V < 2^31, 1 <= F < 2^28, 1 <= R < 2^31.  The
 * specification is restated by ray_mesh_reference of npcd/eval/mesh.py, and the kernel is held to it bit for bit.
 *   npcd_raycast_query: ws as npcd_mesh_distance_boxes of the same (vertices, V, faces, F) left it.  Per ray the lexicographic
 *       minimum of (t, face) over the hits with t_min <= t <= t_max and t < +inf -- t ordered as a signed float with -0 == +0, so
 *       t_min may be negative -- of the watertight ray / triangle test with fp32 sheared corners and float64 edge functions: t [R]
 *       fp32, face [R] int32, bary [R, 3] fp32 (the weights of the face's three corners), front [R] int8 (1: the face's normal
 *       (B - A) x (C - A) points against the ray); (+inf, -1, zeros, 0) for a ray that hits nothing.  cull = 1 skips a tile whose
 *       enlarged box no ray segment of a wave reaches; cull = 0 evaluates every tile.  The outputs are the same bits.  evaluated
 *       (int64 on the device, may be NULL, not zeroed here) takes the (wave, tile) evaluations, one integer add per wave.  One launch.
 * No float atomics, no host synchronisation, no allocation, no workgroup that waits on another.  NPCD_ERR_UNSUPPORTED for V >= 2^31,
 * F >= 2^28 or R >= 2^31; NPCD_ERR_ARG for a negative size, F < 1 or R < 1, a cull that is not 0 or 1, a NULL pointer that the call
 * takes or a misaligned one (ws: 16 bytes, evaluated: 8).  Nothing is launched in either case. */
int npcd_raycast_query(const float* origins, const float* directions, int64_t R, const float* vertices, int64_t V, const int32_t* faces,
                       int64_t F, const void* ws, float t_min, float t_max, int cull, float* t, int32_t* face, float* bary, int8_t* front,
                       int64_t* evaluated, void* stream);

/* ---- how often every ray crosses one mesh, per facing (added within ABI 10; csrc/crossings.hip, csrc/raycast.h).
 * The arrays, their limits and ws are those of npcd_raycast_query.  The specification is restated by crossings_reference of
 * npcd/eval/mesh.py, and the kernel is held to it bit for bit.
 *   npcd_crossings_query: per ray the number of faces it crosses with t_min <= t <= t_max and t < +inf, front [R] int32 those with
 *       det > 0 (the face's normal (B - A) x (C - A) points against the ray) and back [R] int32 those with det < 0.  The corners,
 *       edge functions, det and t are those of npcd_raycast_query; a pair crosses iff each directed edge owns the origin by the
 *       top-left rule, so an edge or a vertex that faces share is crossed once and a face of no projected area never.  A ray that
 *       is not usable gets (0, 0).  cull = 1 skips a tile whose enlarged box no ray segment [t_min, t_max] of a wave reaches; cull
 *       = 0 evaluates every tile.  The outputs are the same counts.  evaluated as for npcd_raycast_query.  One launch.
 * Refusals as for npcd_raycast_query. */
int npcd_crossings_query(const float* origins, const float* directions, int64_t R, const float* vertices, int64_t V, const int32_t* faces,
                         int64_t F, const void* ws, float t_min, float t_max, int cull, int32_t* front, int32_t* back, int64_t* evaluated,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NPCD_HIP_H */
