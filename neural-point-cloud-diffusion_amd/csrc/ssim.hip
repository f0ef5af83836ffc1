// Image metrics of rendered views: the structural similarity index (SSIM) of every (view, channel) and the mean squared
// error of every view, in one pass over the two images.  The operator under npcd.eval.ssim and the ssim= switch of evaluate_pointnerf.
//
//   x = prediction, y = target: fp32, addressed through element strides (view, channel, row, column), so [V, C, H, W] and the renderer's
//   pixel-interleaved [V, H, W, C] are both read where they lie.  A separable window of w taps t (odd, 3 <= w <= 15, float64, sum 1).
//   At the (H - w + 1) (W - w + 1) valid positions, where the window lies inside the image:
//     ux, uy, uxx, uyy, uxy = the window means of x, y, x x, y y, x y with weights t[i] t[j]
//     vx = n (uxx - ux ux), vy = n (uyy - uy uy), vxy = n (uxy - ux uy)
//     S = (2 ux uy + C1)(2 vxy + C2) / ((ux ux + uy uy + C1)(vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2
//   ssim[v, c] = mean of S over the valid positions;  mse[v] = mean of (x - y)^2 over all pixels and channels of the view.
//
// Arithmetic is float64 on the fp32 pixels, every expression evaluated as written (no contraction): uxx - ux ux cancels against
// C2 = 9e-4, and in fp32 the fourth decimal would follow the tiling.  With x == y the numerator and the denominator are the same
// bits, S is 1 exactly and so is its mean.
//
// Launch.  A workgroup of 256 lanes takes one tile of 16 x 32 valid positions of one (view, channel); a grid-stride loop walks the
// tiles.  It stages the tile and its w - 1 halo of both images in LDS as fp32 (30 x 46 at w = 15), runs the horizontal pass into five
// float64 planes (30 x 32 each), then the vertical pass, forms S and sums it.  The squared error is summed while staging, over the
// pixels the tile owns: those of its valid rows and columns, and for the last tile of a row or column the halo behind them as well, so
// every pixel is counted once.  A non-finite pixel adds NaN there (inf - inf and inf^2 would not agree on one), and makes S NaN
// in every window that holds it through inf - inf.  49.5 KB of static LDS, no scratch.
// The two sums of a tile go to a workspace slot of their own, through the fixed float64 tree of wave.h and a fixed order over the four
// waves.  A second small launch adds a view's slots in a fixed order and divides: no float atomics, no fence, the same bits on every
// run, and a view's numbers do not depend on the other views of the call.
//
// Bounds.  The staged rows and columns are r0 + [0, nr + w - 1) with r0 + nr <= H - w + 1: inside the image by construction; every LDS
// index is below the extents of the arrays for w <= 15; the map and the workspace are indexed in 64 bits.
#include "common.h"

namespace npcd {

constexpr int kImThreads = 256, kImWaves = kImThreads / kWave;
constexpr int kImTileR = 16, kImTileC = 32;          // valid positions per workgroup
constexpr int kImMinW = 3, kImMaxW = 15;
constexpr int kImInR = kImTileR + kImMaxW - 1, kImInC = kImTileC + kImMaxW - 1;
constexpr int kImMaxGrid = 1 << 20;

struct ImArgs {
    const float *x, *y;
    int64_t xs[4], ys[4];          // element strides: view, channel, row, column
    const double* taps;            // [w]
    double n, c1, c2;
    double *ws, *map;              // [tiles, 2]; [V, C, H - w + 1, W - w + 1] or NULL
    int C, H, W, w;
    int ntr, ntc;                  // tiles down and across one (view, channel)
    int64_t tiles;                 // V C ntr ntc
};

static inline int im_check(int V, int C, int H, int W, int w) {
    if (V <= 0 || C <= 0 || H <= 0 || W <= 0 || w < kImMinW || w > kImMaxW || !(w & 1) || H < w || W < w) return NPCD_ERR_UNSUPPORTED;
    int64_t count = V;
    for (int d : {C, H, W}) {
        count *= d;
        if (count >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    }
    return NPCD_OK;
}

static inline int64_t im_tiles(int V, int C, int H, int W, int w) {
    return (int64_t)V * C * ceil_div(H - w + 1, kImTileR) * ceil_div(W - w + 1, kImTileC);
}

// both sums over the workgroup, in every lane: the tree of wave.h inside a wave, then the waves in order
__device__ __forceinline__ void im_block_sum2(double& a, double& b, double (*red)[kImWaves], int tid) {
    a = wave_sum_tree(a);
    b = wave_sum_tree(b);
    __syncthreads();          // nobody reads the sums before these any more
    if ((tid & (kWave - 1)) == 0) red[0][tid / kWave] = a, red[1][tid / kWave] = b;
    __syncthreads();
    a = red[0][0], b = red[1][0];
    for (int i = 1; i < kImWaves; ++i) a += red[0][i], b += red[1][i];
}

__global__ __launch_bounds__(kImThreads) void image_metrics_tile_kernel(ImArgs a) {
    __shared__ float sx[kImInR][kImInC], sy[kImInR][kImInC];
    __shared__ double sh[5][kImInR][kImTileC];          // the horizontal pass: x, y, x x, y y, x y
    __shared__ double st[kImMaxW + 1];
    __shared__ double red[2][kImWaves];
    const int tid = threadIdx.x, w = a.w, Hv = a.H - w + 1, Wv = a.W - w + 1, per = a.ntr * a.ntc;
    if (tid < w) st[tid] = a.taps[tid];
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t vc = tile / per;
        const int t = (int)(tile - vc * per), v = (int)(vc / a.C), c = (int)(vc - (int64_t)v * a.C);
        const int tr = t / a.ntc, tc = t - tr * a.ntc, r0 = tr * kImTileR, c0 = tc * kImTileC;
        const int nr = min(kImTileR, Hv - r0), nc = min(kImTileC, Wv - c0), inr = nr + w - 1, inc = nc + w - 1;
        const int own_r = tr == a.ntr - 1 ? inr : kImTileR, own_c = tc == a.ntc - 1 ? inc : kImTileC;
        const float* px = a.x + (v * a.xs[0] + c * a.xs[1] + r0 * a.xs[2] + c0 * a.xs[3]);
        const float* py = a.y + (v * a.ys[0] + c * a.ys[1] + r0 * a.ys[2] + c0 * a.ys[3]);
        __syncthreads();          // the taps are staged; nobody is in the tile before any more
        double err = 0.0;
        for (int i = tid; i < inr * inc; i += kImThreads) {
            const int r = i / inc, q = i - r * inc;
            const float xv = px[r * a.xs[2] + q * a.xs[3]], yv = py[r * a.ys[2] + q * a.ys[3]];
            sx[r][q] = xv, sy[r][q] = yv;
            if (r < own_r && q < own_c) {
                const double d = (double)xv - (double)yv;
                err += fabsf(xv) < INFINITY && fabsf(yv) < INFINITY ? d * d : (double)NAN;
            }
        }
        __syncthreads();
        for (int i = tid; i < inr * kImTileC; i += kImThreads) {
            const int r = i / kImTileC, q = i % kImTileC;
            if (q < nc) {
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
                for (int k = 0; k < w; ++k) {
                    const double tk = st[k], xv = sx[r][q + k], yv = sy[r][q + k];
                    m0 += tk * xv, m1 += tk * yv, m2 += tk * (xv * xv), m3 += tk * (yv * yv), m4 += tk * (xv * yv);
                }
                sh[0][r][q] = m0, sh[1][r][q] = m1, sh[2][r][q] = m2, sh[3][r][q] = m3, sh[4][r][q] = m4;
            }
        }
        __syncthreads();
        double sum = 0.0;
        for (int i = tid; i < nr * kImTileC; i += kImThreads) {
            const int r = i / kImTileC, q = i % kImTileC;
            if (q < nc) {
                double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
                for (int k = 0; k < w; ++k) {
                    const double tk = st[k];
                    ux += tk * sh[0][r + k][q], uy += tk * sh[1][r + k][q], uxx += tk * sh[2][r + k][q], uyy += tk * sh[3][r + k][q],
                        uxy += tk * sh[4][r + k][q];
                }
                const double vx = a.n * (uxx - ux * ux), vy = a.n * (uyy - uy * uy), vxy = a.n * (uxy - ux * uy);
                const double s = ((2.0 * ux * uy + a.c1) * (2.0 * vxy + a.c2)) / ((ux * ux + uy * uy + a.c1) * (vx + vy + a.c2));
                if (a.map) a.map[(vc * Hv + (r0 + r)) * Wv + (c0 + q)] = s;
                sum += s;
            }
        }
        im_block_sum2(sum, err, red, tid);
        if (tid == 0) a.ws[2 * tile] = sum, a.ws[2 * tile + 1] = err;
    }
}

// one workgroup per view: the slots of each channel in a fixed order -> ssim[v, c]; the squared errors of all of them -> mse[v]
__global__ __launch_bounds__(kImThreads) void image_metrics_finish_kernel(const double* __restrict__ ws, double* __restrict__ mse,
                                                                          double* __restrict__ ssim, int V, int C, int per, double valid,
                                                                          double pixels) {
    __shared__ double red[2][kImWaves];
    const int tid = threadIdx.x;
    for (int v = blockIdx.x; v < V; v += gridDim.x) {
        double total = 0.0;
        for (int c = 0; c < C; ++c) {
            const double* slots = ws + 2 * (((int64_t)v * C + c) * per);
            double sum = 0.0, err = 0.0;
            for (int t = tid; t < per; t += kImThreads) sum += slots[2 * t], err += slots[2 * t + 1];
            im_block_sum2(sum, err, red, tid);
            total += err;
            if (tid == 0) ssim[(int64_t)v * C + c] = sum / valid;
        }
        if (tid == 0) mse[v] = total / pixels;
    }
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_image_metrics_tile(int* rows_host, int* cols_host) {
    if (!rows_host || !cols_host) return NPCD_ERR_ARG;
    *rows_host = kImTileR, *cols_host = kImTileC;
    return NPCD_OK;
}

extern "C" int64_t npcd_image_metrics_workspace_bytes(int V, int C, int H, int W, int w) {
    const int rc = im_check(V, C, H, W, w);
    if (rc != NPCD_OK) return rc;
    return im_tiles(V, C, H, W, w) * 2 * (int64_t)sizeof(double);
}

extern "C" int npcd_image_metrics(const float* pred, const float* target, int V, int C, int H, int W, int64_t pred_sv, int64_t pred_sc,
                                  int64_t pred_sh, int64_t pred_sw, int64_t target_sv, int64_t target_sc, int64_t target_sh,
                                  int64_t target_sw, const double* taps, int w, double n, double data_range, double* workspace, double* mse,
                                  double* ssim, double* map, void* stream) {
    const int rc = im_check(V, C, H, W, w);
    if (rc != NPCD_OK) return rc;
    if (!pred || !target || !taps || !workspace || !mse || !ssim || !(data_range > 0.0) || !(data_range < (double)INFINITY) ||
        !(n > 0.0) || !(n < (double)INFINITY))
        return NPCD_ERR_ARG;
    ImArgs a{pred, target, {pred_sv, pred_sc, pred_sh, pred_sw}, {target_sv, target_sc, target_sh, target_sw}, taps, n,
             (0.01 * data_range) * (0.01 * data_range), (0.03 * data_range) * (0.03 * data_range), workspace, map, C, H, W, w,
             ceil_div(H - w + 1, kImTileR), ceil_div(W - w + 1, kImTileC), im_tiles(V, C, H, W, w)};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)(a.tiles < kImMaxGrid ? a.tiles : kImMaxGrid)), dim3(kImThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3((unsigned)(V < kImMaxGrid ? V : kImMaxGrid)), dim3(kImThreads), 0, s, workspace, mse,
                       ssim, V, C, a.ntr * a.ntc, (double)(H - w + 1) * (double)(W - w + 1), (double)C * (double)H * (double)W);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
