// Linear-layer GEMMs of the denoiser block for gfx950, "NT" form:  y[M, N] = x[M, K] . w[N, K]^T (+ bias), 16-bit operands, fp32
// accumulation, 16-bit output -- with the elementwise neighbours of the product fused into its epilogue.
//
// Reference: the nn.Linear forwards of the residual block (transformer.py:67 c_qkv, :107-115 attn.c_proj, :118-137 mlp.c_fc -> GELU
// -> mlp.c_proj, nn.GELU() = exact erf at :131) and, in the backward that autograd derives for them, the data gradients
// dx = dy . W (here: an NT product against the TRANSPOSED 16-bit shadow of W, npcd_transpose_16) followed by the GELU backward.
// Called from the hand-written forward / backward of the fused backbone (npcd/models/diffusion/fused.py).
//
// Why an own kernel, and where it stands (docs/experiments.md R4.1): the library's products run at 1.2-1.3 PF/s at T = 32,768 but leave the
// GELU pair as two separate HBM passes per block (86 + 154 us of a 3.45-ms block).  This family reaches 0.85-0.9 x the tuned library on
// the bare products (c_fc 259 against 211-237 us) and 384 against 420-440 us for the data gradient of mlp.c_proj WITH the GELU backward
// and the bias-gradient sums in its epilogue -- parity inside the step, hence an opt-in of the backbone (NPCD_OWN_DGELU=1).  The wall
// both stand at: a 256 x 256 bf16 tile asks the CU for 32 bytes per clock of LDS fill (one 1-KB request per ~32 cycles is what its
// vector-memory path takes) AND for all of its matrix pipe; pipe busy 0.51 here, 0.62 in the library's stream-K kernel.
//
// Structure (one workgroup = 8 waves = one 256 x 256 output tile, PERSISTENT over a static list of tiles):
//   * both operands are K-contiguous, so a K-step of 64 is 256 + 256 rows of 128 bytes, moved as two 32-KB HALF-stages (x rows, w rows)
//     by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction = 8 rows; the XOR swizzle of the 16-byte chunk index is applied
//     to the SOURCE address, the LDS image stays lane-linear) and read back with ds_read_b128 (conflict-free row reads, common.h);
//   * a ring of FIVE half-stage buffers = the CU's 160 KB: the x stream runs two steps ahead, the w stream one, the request queue
//     never runs empty at a barrier, and the stream runs across tile boundaries (the next tile's first steps land during the epilogue);
//   * loader roles: waves 4..7 request the w half-stage (8 pieces each, right behind the step's barrier), waves 0..3 the x half-stage
//     (behind the matrix instructions of the next step's sub-steps): a request blocks its wave for 115-170 cycles, and this way one
//     wave of every SIMD issues matrix instructions meanwhile;
//   * wave (wm, wn) owns rows [128 wm, +128) x columns [64 wn, +64): 8 accumulators of 32 x 32 (v_mfma_f32_32x32x16), oriented
//     with the OUTPUT COLUMN on the accumulator row (registers) and the output row on the lane: a lane then holds runs of four
//     consecutive columns of one output row, two runs are joined by v_permlane32_swap into 16-byte stores, the bias is the same for
//     all lanes of a register (no LDS transpose: there is no LDS left);
//   * tile order: 8 (row) x 4 (column) super-tiles, one per XCD and round (workgroups b, b + 8, ... share an XCD and its L2), so
//     that the 32 tiles an XCD works on at a time read 8 + 4 operand panels instead of 32 + 32.
#include <type_traits>

#include "common.h"

namespace npcd {

__device__ __forceinline__ uint32_t l_lds_addr(const unsigned char* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char*)p;
}
__device__ __forceinline__ const void* l_uniform_ptr(const void* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const void*>(((uint64_t)hi << 32) | lo);
}
// one LDS-DMA wave-instruction: wave-uniform 64-bit base + one 32-bit byte offset per lane -> LDS (M0 = wave-uniform destination)
__device__ __forceinline__ void l_dma16(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    sbase = l_uniform_ptr(sbase);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// the same with a 64-bit address per lane (ragged ends)
__device__ __forceinline__ void l_dma16_lane(const void* src, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_dst) : "memory");
}
template <int OFF>
__device__ __forceinline__ u32x4 l_rd128(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}

enum { LIN_PLAIN = 0, LIN_GELU = 1, LIN_DGELU = 2 };

#ifdef NPCD_LIN_TL
// DIAGNOSTIC build only (tools/probes/gpu_dev_lin_timeline.py): s_memtime stamps of ONE K-step (global step NPCD_LIN_TL of workgroup 0)
// of waves 0 and 4, read back with npcd_lin_debug_read.  Instrumentation costs ~10 % of the wave's cycles.
__device__ long long g_lin_tl[2][32];
#define NPCD_LTS(i)                                                           \
    do {                                                                      \
        if (tl_on) {                                                          \
            __builtin_amdgcn_sched_barrier(0);                                \
            tl[(i)] = __builtin_amdgcn_s_memtime();                           \
            __builtin_amdgcn_sched_barrier(0);                                \
        }                                                                     \
    } while (0)
#else
#define NPCD_LTS(i) do { } while (0)
#endif

struct LinParams {
    const void* x;        // [M, K]
    const void* w;        // [N, K]
    const void* bias;     // [N] (16 bit) or nullptr
    void* y;              // [M, N]
    void* y2;             // LIN_GELU: gelu(y) [M, N]
    const void* aux;      // LIN_DGELU: the pre-activation h [M, N]
    float* part;          // LIN_DGELU: column partial sums [tiles_m][N]
    int M, N, K;
    int tiles_m, tiles_n, ntiles;
    int full_m;           // row tiles covered by 8 x 4 super-tiles (a multiple of 8); the rest are ordered column-fastest
};

#ifndef NPCD_LIN_DIAG
#define NPCD_LIN_DIAG 0        // DIAGNOSTIC builds (wrong results, timing only): 1 no DMA inside the loop, 2 no matrix instructions,
                               // 3 no epilogue stores, 4 neither matrix instructions nor fragment reads
#endif
// Issue schedule of an x loader's 8 LDS-DMA instructions per step: X0 / X1 / X2 behind the matrix instructions of K-sub-steps 0 / 1 / 2
// (X0 + X1 <= 8; the rest in sub-step 2).  The w loaders issue their 8 right behind the barrier.
#ifndef NPCD_LIN_X0
#define NPCD_LIN_X0 4
#define NPCD_LIN_X1 4
#endif
static_assert(NPCD_LIN_X0 + NPCD_LIN_X1 <= 8, "an x loader issues 8 DMA instructions per step");

constexpr int kLBuf = 32768;           // one ring buffer = a half-stage: x rows [256][64] or w rows [256][64] of a K-step
constexpr int kLRing = 5 * kLBuf;      // 160 KiB: all of a CU's LDS

// logical tile index -> (row tile, column tile)
__device__ __forceinline__ void lin_tile(const LinParams& p, int l, int& tm, int& tn) {
    const int sup = p.full_m * p.tiles_n;
    if (l < sup) {
        const int gn = p.tiles_n >> 2, grp = l >> 5, in = l & 31;
        tn = (grp % gn) * 4 + (in & 3);
        tm = (grp / gn) * 8 + (in >> 2);
    } else {
        l -= sup;
        tn = l % p.tiles_n;
        tm = p.full_m + l / p.tiles_n;
    }
}

// branch-free Phi(x) (Abramowitz & Stegun 7.1.26, |error| <= 7.5e-8; the formula of csrc/elementwise.hip): gelu(x) = x Phi(x)
__device__ __forceinline__ float lin_gelu(float x) {
    const float u = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, u, 1.f));
    const float e = __builtin_amdgcn_exp2f(x * x * -0.72134752044448170f);
    float poly = __builtin_fmaf(t, 1.061405429f, -1.453152027f);
    poly = __builtin_fmaf(poly, t, 1.421413741f);
    poly = __builtin_fmaf(poly, t, -0.284496736f);
    poly = __builtin_fmaf(poly, t, 0.254829592f);
    const float erf_abs = __builtin_fmaf(-poly * t, e, 1.f);
    return x * __builtin_fmaf(0.5f, copysignf(erf_abs, x), 0.5f);
}
__device__ __forceinline__ float lin_gelu_grad(float x) {
    const float u = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, u, 1.f));
    const float e = __builtin_amdgcn_exp2f(x * x * -0.72134752044448170f);          // exp(-x^2 / 2)
    float poly = __builtin_fmaf(t, 1.061405429f, -1.453152027f);
    poly = __builtin_fmaf(poly, t, 1.421413741f);
    poly = __builtin_fmaf(poly, t, -0.284496736f);
    poly = __builtin_fmaf(poly, t, 0.254829592f);
    const float erf_abs = __builtin_fmaf(-poly * t, e, 1.f);
    const float phi_cdf = __builtin_fmaf(0.5f, copysignf(erf_abs, x), 0.5f);
    return __builtin_fmaf(x * 0.3989422804014327f, e, phi_cdf);
}

template <class E>
__device__ __forceinline__ uint32_t lin_pack2(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) E e2;
    const e2 t = {(E)a, (E)b};
    return __builtin_bit_cast(uint32_t, t);
}
template <class TR>
__device__ __forceinline__ void lin_unpack4(const u32x2 v, float (&f)[4]) {
    f[0] = TR::lo(v[0]); f[1] = TR::hi(v[0]); f[2] = TR::lo(v[1]); f[3] = TR::hi(v[1]);
}

template <class TR, int EPI>
__global__ __launch_bounds__(512, 2) void lin_kernel(LinParams p) {
    using E = typename TR::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // 2 stages x 64 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;                                   // wave tile: rows [128 wm, +128) x columns [64 wn, +64)
    const int G = gridDim.x;
    const int me = xcd_remap(blockIdx.x, G);                                   // position inside a round: an XCD's workgroups are consecutive
    const int nk = p.K >> 6;
    const E* X = static_cast<const E*>(p.x);
    const E* W = static_cast<const E*>(p.w);
    const uint32_t lds0 = l_lds_addr(smem);

    // ---- DMA stream: HALF-stages (the x rows [256][64] of a K-step: even numbers h = 2 g; its w rows: odd, h = 2 g + 1; 32 KB each)
    // through a ring of FIVE buffers, half-stage h in buffer h % 5.  When step g has been read, half-stages 2 g + 5 (w of step g + 2:
    // needed at the END of the next step, "urgent") and 2 g + 6 (x of step g + 3: a step more to land) are requested, so the queue
    // never runs empty at a barrier.  ROLES: waves 4..7 request the w half-stages (8 pieces of 8 rows each, all right behind the
    // barrier), waves 0..3 the x half-stages (8 pieces, spread behind the matrix instructions of the next step's sub-steps) -- the
    // two waves of a SIMD (w and w + 4) are then never both stuck in DMA issue: one issues matrix instructions meanwhile.
    const int rowin = lane >> 3;
    const bool ldw = wave >= 4;
    const int lw = wave & 3;                                                   // rows [64 lw, +64) of the half-stage
    uint32_t voff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) voff[i] = (uint32_t)((rowin * p.K + (((lane & 7) ^ tile_swz(8 * i + rowin)) << 3)) * (int)sizeof(E));
    int d_tile = me, d_kt = 0, d_row0 = 0;                                     // cursor of THIS wave's stream: tile, K-step, first row / column
    uint32_t d_buf = ldw ? kLBuf : 0;                                          // byte offset of the buffer the cursor's half-stage goes to
    int tail_real = 0;                                                         // was the most recently requested half-stage a real one?
    int dma_on = 1;                                                            // (off during the very first step: its requests are the prologue's)
    {
        int tm, tn;
        lin_tile(p, d_tile < p.ntiles ? d_tile : 0, tm, tn);
        d_row0 = (ldw ? tn : tm) * 256;
    }
    auto dma_piece = [&](int i) {                                              // piece i = 0..7 of the half-stage under the cursor
        if (d_tile >= p.ntiles) return;
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + d_buf + (64 * lw + 8 * i) * 128);
        const int row0 = d_row0 + 64 * lw + 8 * i;
        if (ldw) {
            l_dma16(W + (int64_t)row0 * p.K + d_kt * 64, voff[i & 1], dst);
        } else if (row0 + 8 <= p.M) {
            l_dma16(X + (int64_t)row0 * p.K + d_kt * 64, voff[i & 1], dst);
        } else {                                                               // ragged end of M: rows past it re-read the last row (never stored)
            const int row = min(row0 + rowin, p.M - 1);
            l_dma16_lane(X + (int64_t)row * p.K + d_kt * 64 + (((lane & 7) ^ tile_swz(8 * i + rowin)) << 3), dst);
        }
    };
    auto dma_half_done = [&]() {
        tail_real = d_tile < p.ntiles;
        d_buf = d_buf >= 3 * kLBuf ? d_buf - 3 * kLBuf : d_buf + 2 * kLBuf;   // (h + 2) % 5
        if (++d_kt == nk) {
            d_kt = 0;
            d_tile += G;
            if (d_tile < p.ntiles) {
                int tm, tn;
                lin_tile(p, d_tile, tm, tn);
                d_row0 = (ldw ? tn : tm) * 256;
            }
        }
    };
    // pieces [LO, HI) of the 8 a wave requests per step
#define NPCD_L_DMA(LO, HI)                                                 \
    do {                                                                   \
        if (NPCD_LIN_DIAG == 1 || !dma_on) break;                          \
        _Pragma("unroll") for (int q = (LO); q < (HI); ++q) dma_piece(q);  \
        if ((HI) == 8 && (LO) < (HI)) dma_half_done();                     \
    } while (0)

    // ---- fragment addresses: MFMA operand lane (r, h) reads row r, 16-byte chunk 2 s + h of K-sub-step s
    const int r = lane & 31, h = lane >> 5;
    uint32_t xa[4], wa[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t c = (uint32_t)(((2 * s + h) ^ tile_swz(r)) << 4);
        xa[s] = lds0 + (128 * wm + r) * 128 + c;
        wa[s] = lds0 + (64 * wn + r) * 128 + c;
    }

    f32x16 acc[2][4];          // [column block ni][row block mi]: accumulator row = output column, lane = output row
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x16{0};

#define NPCD_L_VMWAIT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
#define NPCD_L_WAIT()                                       \
    do {                                                    \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        __builtin_amdgcn_sched_barrier(0);                  \
    } while (0)
#define NPCD_L_ISSUE(FX, FW, OX, OW, S)                                                           \
    do {                                                                                          \
        if (NPCD_LIN_DIAG == 4) break;                                                            \
        FX[0] = l_rd128<0>(xa[S] + (OX));     FX[1] = l_rd128<4096>(xa[S] + (OX));                \
        FX[2] = l_rd128<8192>(xa[S] + (OX));  FX[3] = l_rd128<12288>(xa[S] + (OX));               \
        FW[0] = l_rd128<0>(wa[S] + (OW));     FW[1] = l_rd128<4096>(wa[S] + (OW));                \
    } while (0)
#define NPCD_L_MMA(FX, FW)                                                                        \
    do {                                                                                          \
        _Pragma("unroll") for (int ni = 0; ni < 2; ++ni)                                          \
            _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                      \
                if (NPCD_LIN_DIAG != 2 && NPCD_LIN_DIAG != 4)                                     \
                    acc[ni][mi] = TR::mfma32(__builtin_bit_cast(typename TR::vec8, FW[ni]), __builtin_bit_cast(typename TR::vec8, FX[mi]), acc[ni][mi]); \
                else if (NPCD_LIN_DIAG == 2) acc[ni][mi][0] += __uint_as_float(FW[ni][0] ^ FX[mi][3]); \
    } while (0)

    if (me >= p.ntiles) return;
    // ---- prologue: half-stages 0 .. 4 (x loaders: 0, 2, 4; w loaders: 1, 3); 0 and 1 must have landed
    NPCD_L_DMA(0, 8);
    {
        int extra = 0;                                                         // this wave's real half-stages beyond the first
        NPCD_L_DMA(0, 8); extra += tail_real;
        if (!ldw) { NPCD_L_DMA(0, 8); extra += tail_real; }
        if (extra == 2) NPCD_L_VMWAIT(16);
        else if (extra == 1) NPCD_L_VMWAIT(8);
        else NPCD_L_VMWAIT(0);
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    dma_on = 0;                                          // a round of 8 pieces starts BEHIND a step's barrier and ends in the next step's sub-steps
#ifdef NPCD_LIN_TL
    long long tl[19];
    for (int i = 0; i < 19; ++i) tl[i] = 0;
    int gstep = 0;
#endif
    u32x4 fx0[4] = {}, fw0[2] = {}, fx1[4] = {}, fw1[2] = {};
    uint32_t ox = 0, ow = kLBuf;                         // LDS offsets of the buffers being read: half-stages 2 g and 2 g + 1
    NPCD_L_ISSUE(fx0, fw0, ox, ow, 0);
    for (int tile = me; tile < p.ntiles; tile += G) {
        int tm, tn;
        lin_tile(p, tile, tm, tn);
        const int m0 = tm * 256, n0 = tn * 256;
        for (int kt = 0; kt < nk; ++kt) {
#ifdef NPCD_LIN_TL
            const bool tl_on = blockIdx.x == 0 && (wave == 0 || wave == 4) && gstep == NPCD_LIN_TL;
            ++gstep;
#endif
            // (the 8 pieces requested in this step were freed by the previous step: P3 behind its barrier, P0 / P1 / P2 here)
            // sub-step 0
            NPCD_LTS(0);
            NPCD_L_WAIT();
            NPCD_LTS(1);
            NPCD_L_ISSUE(fx1, fw1, ox, ow, 1);
            NPCD_LTS(2);
            NPCD_L_MMA(fx0, fw0);
            NPCD_LTS(3);
            if (!ldw) NPCD_L_DMA(0, NPCD_LIN_X0);
            // sub-step 1
            NPCD_LTS(4);
            NPCD_L_WAIT();
            NPCD_LTS(5);
            NPCD_L_ISSUE(fx0, fw0, ox, ow, 2);
            NPCD_LTS(6);
            NPCD_L_MMA(fx1, fw1);
            NPCD_LTS(7);
            if (!ldw) NPCD_L_DMA(NPCD_LIN_X0, NPCD_LIN_X0 + NPCD_LIN_X1);
            // sub-step 2
            NPCD_LTS(8);
            NPCD_L_WAIT();
            NPCD_LTS(9);
            NPCD_L_ISSUE(fx1, fw1, ox, ow, 3);
            NPCD_LTS(10);
            NPCD_L_MMA(fx0, fw0);
            NPCD_LTS(11);
            if (!ldw) NPCD_L_DMA(NPCD_LIN_X0 + NPCD_LIN_X1, 8);
            // sub-step 3: this wave has read everything of the step; the next step's two half-stages must have landed for everybody
            // (an x loader's half-stage requested last may stay in flight: it belongs to the step after the next)
            NPCD_LTS(12);
            NPCD_L_WAIT();
            NPCD_LTS(13);
            if (!ldw && tail_real) NPCD_L_VMWAIT(8);
            else NPCD_L_VMWAIT(0);
            NPCD_LTS(14);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            NPCD_LTS(15);
            // the two buffers just read are free: half-stages 2 g + 5 (w, now) and 2 g + 6 (x, during the next step) go into them
            dma_on = 1;
            if (ldw) NPCD_L_DMA(0, 8);
            NPCD_LTS(16);
            ox = ox >= 3 * kLBuf ? ox - 3 * kLBuf : ox + 2 * kLBuf;
            ow = ow >= 3 * kLBuf ? ow - 3 * kLBuf : ow + 2 * kLBuf;
            NPCD_L_ISSUE(fx0, fw0, ox, ow, 0);           // first fragments of the next step (possibly the next tile's)
            NPCD_LTS(17);
            NPCD_L_MMA(fx1, fw1);
            NPCD_LTS(18);
#ifdef NPCD_LIN_TL
            if (tl_on && lane == 0)
                for (int i = 0; i < 19; ++i) g_lin_tl[wave >> 2][i] = tl[i];
#endif
        }
        // ---- epilogue of the tile: lane = output row, register quads = 4 consecutive output columns
        if (NPCD_LIN_DIAG == 3 && acc[0][0][0] != 12345.678f) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x16{0};
            continue;
        }
        const E* bias = static_cast<const E*>(p.bias);
        E* Y = static_cast<E*>(p.y);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int nb = n0 + 64 * wn + 32 * ni;
            float bq[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (bias) lin_unpack4<TR>(*reinterpret_cast<const u32x2*>(bias + nb + 8 * q + 4 * h), bq[q]);
                else bq[q][0] = bq[q][1] = bq[q][2] = bq[q][3] = 0.f;
            }
            float csum[4][4];                                                   // LIN_DGELU: column sums of this lane's rows
            if (EPI == LIN_DGELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) csum[q][0] = csum[q][1] = csum[q][2] = csum[q][3] = 0.f;
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int m = m0 + 128 * wm + 32 * mi + r;
                const bool ok = m < p.M;
                const int64_t rowoff = (int64_t)(ok ? m : 0) * p.N + nb + 8 * h;
#pragma unroll
                for (int qp = 0; qp < 2; ++qp) {
                    float v[2][4];
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[e][j] = acc[ni][mi][4 * (2 * qp + e) + j] + bq[2 * qp + e][j];
                    uint32_t a0 = lin_pack2<E>(v[0][0], v[0][1]), a1 = lin_pack2<E>(v[0][2], v[0][3]);
                    uint32_t b0 = lin_pack2<E>(v[1][0], v[1][1]), b1 = lin_pack2<E>(v[1][2], v[1][3]);
                    if (EPI == LIN_DGELU) {
                        // dh = round16(dg) * gelu'(h): h at THIS lane's pre-swap positions (columns nb + 8 q + 4 h + j of row m)
                        const E* hp = static_cast<const E*>(p.aux) + (int64_t)(ok ? m : 0) * p.N + nb + 16 * qp + 4 * h;
                        float h0[4], h1[4], d0[4], d1[4];
                        lin_unpack4<TR>(*reinterpret_cast<const u32x2*>(hp), h0);
                        lin_unpack4<TR>(*reinterpret_cast<const u32x2*>(hp + 8), h1);
                        lin_unpack4<TR>(u32x2{a0, a1}, d0);
                        lin_unpack4<TR>(u32x2{b0, b1}, d1);
                        float o0[4], o1[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            o0[j] = (float)(E)(d0[j] * lin_gelu_grad(h0[j]));
                            o1[j] = (float)(E)(d1[j] * lin_gelu_grad(h1[j]));
                            if (ok) { csum[2 * qp][j] += o0[j]; csum[2 * qp + 1][j] += o1[j]; }
                        }
                        a0 = lin_pack2<E>(o0[0], o0[1]); a1 = lin_pack2<E>(o0[2], o0[3]);
                        b0 = lin_pack2<E>(o1[0], o1[1]); b1 = lin_pack2<E>(o1[2], o1[3]);
                    }
                    uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0;
                    if (EPI == LIN_GELU) {
                        float t0[4], t1[4];
                        lin_unpack4<TR>(u32x2{a0, a1}, t0);                    // gelu of the ROUNDED pre-activation, like the reference
                        lin_unpack4<TR>(u32x2{b0, b1}, t1);
                        g0 = lin_pack2<E>(lin_gelu(t0[0]), lin_gelu(t0[1])); g1 = lin_pack2<E>(lin_gelu(t0[2]), lin_gelu(t0[3]));
                        g2 = lin_pack2<E>(lin_gelu(t1[0]), lin_gelu(t1[1])); g3 = lin_pack2<E>(lin_gelu(t1[2]), lin_gelu(t1[3]));
                    }
                    // lanes l and l + 32 hold columns 4 h + j of the same row: after the half-swap a lane holds 8 consecutive columns
                    auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
                    auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
                    if (ok) *reinterpret_cast<u32x4*>(Y + rowoff + 16 * qp) = u32x4{s0[0], s1[0], s0[1], s1[1]};
                    if (EPI == LIN_GELU) {
                        auto s2 = __builtin_amdgcn_permlane32_swap(g0, g2, false, false);
                        auto s3 = __builtin_amdgcn_permlane32_swap(g1, g3, false, false);
                        if (ok) *reinterpret_cast<u32x4*>(static_cast<E*>(p.y2) + rowoff + 16 * qp) = u32x4{s2[0], s3[0], s2[1], s3[1]};
                    }
                }
                acc[ni][mi] = f32x16{0};
            }
            if (EPI == LIN_DGELU) {
                // column sums over this wave's 128 rows: lanes of one half add up (32 rows each x 4 row blocks were added above)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float sres = csum[q][j];
#pragma unroll
                        for (int o = 16; o >= 1; o >>= 1) sres += __shfl_xor(sres, o, 64);
                        csum[q][j] = sres;
                    }
                // one fp32 row of partial sums per (row tile, wave row wm): part[(2 tm + wm)][N]
                if (r == 0) {
                    float* pp = p.part + (int64_t)(2 * tm + wm) * p.N + nb + 4 * h;
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(pp + 8 * q) = f32x4{csum[q][0], csum[q][1], csum[q][2], csum[q][3]};
                }
            }
        }
    }
#undef NPCD_L_ISSUE
#undef NPCD_L_DMA
#undef NPCD_L_MMA
#undef NPCD_L_WAIT
#undef NPCD_L_VMWAIT
}

// ============================================================================================================================
// Small-M form: 128 x 128 tiles.  At the token counts of a rank of the 4- / 8-GPU job (T = 8,208 / 4,104) the
// N = 1,024 products of a block have 64-68 tiles of 256 x 256 on 256 CUs; with 128 x 128 tiles they have 264 / 520.  One workgroup
// per tile (8 waves on four 64 x 64 wave tiles), K-steps of 64 through three LDS stages filled global -> registers -> LDS, one barrier
// per K-step (LDS-DMA is not used here: with one wave per SIMD -- 264 workgroups on 256 CUs -- its 115-170 blocked issue cycles per
// instruction, R4.1, would exceed the step's 512 matrix cycles).  The LAST row tile takes up to 160 rows (M mod 128 <= 32: the 8 / 16 /
// 32 rows of the time-step tokens would otherwise be a second round of 8 workgroups on a full chip): its upper waves carry a third
// row block.  Bound: LDS traffic -- per K-step and CU 64 KB of fragment reads + 32 KB of stage writes against 512 matrix cycles.
#ifdef NPCD_L128_TL
__device__ long long g_l128_tl[2][12];
#endif
struct Lin128Params {
    const void* x; const void* w; const void* bias; void* y;
    int M, N, K, tiles_m, tiles_n;
    int tall;             // rows of the last row tile (128 < tall <= 160), or 0: all row tiles have <= 128 rows
};
constexpr int kL128Rows = 160;                                   // x rows of a stage (the tall tile's)
constexpr int kL128Stage = (kL128Rows + 128) * 128;              // bytes: x rows [160][64] + w rows [128][64]
constexpr int kL128Lds = 3 * kL128Stage;                         // 110,592 B: one workgroup (eight waves) per CU

template <class TR, int MB1>          // MB1 = row blocks of the upper waves (wm = 1): 2, or 3 in the tall last row tile
__device__ __forceinline__ void lin128_tile(const Lin128Params& p, unsigned char* smem, int tm, int tn) {
    using E = typename TR::elem;
    constexpr int XL = MB1 == 3 ? 3 : 2;                           // 16-byte loads per thread and stage for the x rows (rows lrow + 64 i)
    constexpr int MB = MB1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // EIGHT waves on a tile of four 64 x 64 wave tiles: waves w and w + 4 share a wave tile and split every K-step's four sub-steps
    // (kg = 0: sub-steps 0, 1; kg = 1: 2, 3), their partial accumulators meet through LDS at the end.  Two waves per SIMD from ONE
    // workgroup per CU (264 workgroups on 256 CUs): as four waves the loop ran at the latency of its own LDS reads and load waits
    // (1,450 clocks per K-step without any stage traffic against 512 of matrix instructions).
    const int kg = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;
    const int nk = p.K >> 6, m0 = tm * 128, n0 = tn * 128;
    const E* X = static_cast<const E*>(p.x);
    const E* W = static_cast<const E*>(p.w);
    // ---- global -> register staging: thread t takes 16-byte chunk (t & 7) of rows (t >> 3) + 64 i
    const int lrow = tid >> 3, lchunk = tid & 7;
    // (raw buffer loads: per-thread byte offset + a scalar offset per K-step -- as 64-bit `global_load` addresses the compiler rebuilt
    // them in front of every load IN the destination registers of the loads still in flight, i.e. waited for those first)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<E*>(X), 0, (int)min((int64_t)p.M * p.K * 2, (int64_t)0x7fffffff), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<E*>(W), 0, (int)min((int64_t)p.N * p.K * 2, (int64_t)0x7fffffff), 0x00020000);
    int xo[XL], wo[2];
#pragma unroll
    for (int i = 0; i < XL; ++i) xo[i] = (min(m0 + lrow + 64 * i, p.M - 1) * p.K + lchunk * 8) * 2;     // rows past M re-read the last one
#pragma unroll
    for (int i = 0; i < 2; ++i) wo[i] = ((n0 + lrow + 64 * i) * p.K + lchunk * 8) * 2;
    const uint32_t lds0 = l_lds_addr(smem);
    const uint32_t st_off = (uint32_t)tile_off(lrow, lchunk);                  // (rows r and r + 64 i share the swizzle: it repeats every 8 rows)
    const bool x2_ok = MB1 == 3 && lrow < kL128Rows - 128;                       // the tall tile's third group: rows 128 .. 159 only
    // two register sets: stage s is requested at the top of step s - 2 and written to LDS at the top of step s - 1 (its buffer, s & 1,
    // was last read in step s - 2): two K-steps of flight time
    u32x4 gx[2][XL], gw[2][2];
    auto g_load = [&](int set, int kt) {
#pragma unroll
        for (int i = 0; i < XL; ++i) gx[set][i] = __builtin_amdgcn_raw_buffer_load_b128(rx, xo[i], kt * 128, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) gw[set][i] = __builtin_amdgcn_raw_buffer_load_b128(rw, wo[i], kt * 128, 0);
    };
    auto s_store = [&](int set, int buf) {
        unsigned char* b = smem + buf * kL128Stage;
#pragma unroll
        for (int i = 0; i < XL; ++i)
            if (i < 2 || x2_ok) *reinterpret_cast<u32x4*>(b + st_off + i * 64 * 128) = gx[set][i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(b + kL128Rows * 128 + st_off + i * 64 * 128) = gw[set][i];
    };
    // ---- fragment addresses: MFMA operand lane (r, h) reads row r, 16-byte chunk 2 s + h of K-sub-step s = 2 kg + j
    const int r = lane & 31, h = lane >> 5;
    // tall tile: BOTH wave rows carry three blocks, rows [0, 96) and [64, 160) -- the lower waves' third block repeats rows the upper
    // ones own and is never stored: a wave-uniform `if (block < mine)` around every matrix instruction cut the loop into single-instruction
    // basic blocks
    const int mb_store = (MB1 == 3 && wm == 0) ? 2 : MB1;
    const int xrow0 = 64 * wm;
    uint32_t xa[2], wa[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t c = (uint32_t)(((2 * (2 * kg + j) + h) ^ tile_swz(r)) << 4);
        xa[j] = (xrow0 + r) * 128 + c;
        wa[j] = kL128Rows * 128 + (64 * wn + r) * 128 + c;
    }
    f32x16 acc[2][MB];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) acc[ni][mi] = f32x16{0};

#ifndef NPCD_L128_DIAG
#define NPCD_L128_DIAG 0          // DIAGNOSTIC builds (wrong results, timing only): 1 no global loads in the loop, 2 no matrix instructions, 3 no stage writes
#endif
    // Pipeline over THREE LDS stages.  Stage u: global -> registers in step u - 3, registers -> LDS (buffer u % 3) in step u - 2,
    // complete behind that step's barrier, its fragments are read during the matrix instructions of step u - 1, multiplied in
    // step u.  One barrier per step; a wave's LDS reads always run one step ahead of its matrix instructions.
    u32x4 fx[2][2][MB], fw[2][2][2];                    // [parity of the step][sub-step j][block]
    auto f_read = [&](int par, uint32_t bo) {
        const unsigned char* sb = smem + bo;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int mi = 0; mi < MB; ++mi)
                fx[par][j][mi] = *reinterpret_cast<const u32x4*>(sb + xa[j] + mi * 4096);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) fw[par][j][ni] = *reinterpret_cast<const u32x4*>(sb + wa[j] + ni * 4096);
        }
    };
    auto k_mma = [&](int par) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < MB; ++mi) {
                    if (NPCD_L128_DIAG != 2) acc[ni][mi] = TR::mfma32(__builtin_bit_cast(typename TR::vec8, fw[par][j][ni]), __builtin_bit_cast(typename TR::vec8, fx[par][j][mi]), acc[ni][mi]);
                    else acc[ni][mi][0] += __uint_as_float(fw[par][j][ni][0] ^ fx[par][j][mi][3]);
                }
    };
    // prologue: stages 0 and 1 in LDS, stage 2 in registers (set 0), the fragments of step 0 read
    g_load(0, 0);
    if (nk > 1) g_load(1, 1);
    s_store(0, 0);
    if (nk > 2) g_load(0, 2);
    if (nk > 1) s_store(1, 1);
    __syncthreads();
    f_read(0, 0);
    uint32_t b_cur = 0;                                  // byte offset of the buffer of the step being multiplied
    auto nxt = [](uint32_t b) { return b == 2 * kL128Stage ? 0u : b + (uint32_t)kL128Stage; };
    // steps in pairs: the register set of a stage (its parity) and the fragment set of a step are compile-time choices.  The steady
    // state (four more stages exist) runs without conditions; the last two pairs take the guarded form.
#ifdef NPCD_L128_TL
    // DIAGNOSTIC build: s_memtime stamps of the step pair kt = NPCD_L128_TL of workgroup 0, waves 0 and 4 (npcd_lin128_debug_read)
    long long tl[12];
    for (int i = 0; i < 12; ++i) tl[i] = 0;
#define NPCD_L8S(i) do { if (tl_on) { __builtin_amdgcn_sched_barrier(0); tl[(i)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define NPCD_L8S(i) do { } while (0)
#endif
    auto step_pair = [&](int kt, auto guarded) {
        constexpr bool G = decltype(guarded)::value;
#ifdef NPCD_L128_TL
        const bool tl_on = blockIdx.x == 0 && (wave == 0 || wave == 4) && kt == NPCD_L128_TL;
#endif
        const uint32_t b1 = nxt(b_cur), b2 = nxt(b1);
        // (the request for stage kt + 3 goes out BEFORE the wait for stage kt + 2: the wait then leaves the newest loads in flight)
        // order inside a step (pinned: left alone the compiler moved the matrix instructions BELOW the barrier, behind a full
        // `lgkmcnt(0)` drain of the stage writes and the next step's fragment reads): requests, fragment reads of the next step,
        // matrix instructions, and only then the wait for the stage in flight + its LDS writes -- they run under the matrix pipe
        NPCD_L8S(0);
        if (NPCD_L128_DIAG != 1 && (!G || kt + 3 < nk)) g_load(1, kt + 3);
        NPCD_L8S(1);
        if (!G || kt + 1 < nk) f_read(1, b1);
        __builtin_amdgcn_sched_barrier(0);
        NPCD_L8S(2);
        k_mma(0);
        __builtin_amdgcn_sched_barrier(0);
        NPCD_L8S(3);
        if (NPCD_L128_DIAG != 3 && (!G || kt + 2 < nk)) s_store(0, (int)(b2 / kL128Stage));
        NPCD_L8S(4);
        __syncthreads();
        NPCD_L8S(5);
        if (!G || kt + 1 < nk) {
            if (NPCD_L128_DIAG != 1 && (!G || kt + 4 < nk)) g_load(0, kt + 4);
            NPCD_L8S(6);
            if (!G || kt + 2 < nk) f_read(0, b2);
            __builtin_amdgcn_sched_barrier(0);
            NPCD_L8S(7);
            k_mma(1);
            __builtin_amdgcn_sched_barrier(0);
            NPCD_L8S(8);
            if (NPCD_L128_DIAG != 3 && (!G || kt + 3 < nk)) s_store(1, (int)(b_cur / kL128Stage));      // buffer (kt + 3) % 3 = the one of step kt
            NPCD_L8S(9);
            __syncthreads();
            NPCD_L8S(10);
        }
#ifdef NPCD_L128_TL
        if (tl_on && lane == 0)
            for (int i = 0; i < 12; ++i) g_l128_tl[wave >> 2][i] = tl[i];
#endif
        b_cur = b2;
    };
    int kt = 0;
    for (; kt + 4 < nk; kt += 2) step_pair(kt, std::false_type{});
    for (; kt < nk; kt += 2) step_pair(kt, std::true_type{});
    // ---- the two halves of every K-step meet: the upper waves hand their partial accumulators over through LDS (one column block
    // at a time: <= 40 KB), the lower waves add them and write the tile
    {
        float* red = reinterpret_cast<float*>(smem) + ((wave & 3) * (MB * 16) * 64 + lane) * 1;      // [wave tile][register][lane]
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if (kg == 1) {
#pragma unroll
                for (int mi = 0; mi < MB; ++mi)
#pragma unroll
                    for (int e = 0; e < 16; ++e) red[(mi * 16 + e) * 64] = acc[ni][mi][e];
            }
            __syncthreads();
            if (kg == 0) {
#pragma unroll
                for (int mi = 0; mi < MB; ++mi)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[ni][mi][e] += red[(mi * 16 + e) * 64];
            }
            __syncthreads();
        }
    }
    if (kg == 1) return;
    // ---- epilogue: lane = output row, register quads = 4 consecutive output columns; lanes l and l + 32 joined into 16-byte stores
    const E* bias = static_cast<const E*>(p.bias);
    E* Y = static_cast<E*>(p.y);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int nb = n0 + 64 * wn + 32 * ni;
        float bq[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (bias) lin_unpack4<TR>(*reinterpret_cast<const u32x2*>(bias + nb + 8 * q + 4 * h), bq[q]);
            else bq[q][0] = bq[q][1] = bq[q][2] = bq[q][3] = 0.f;
        }
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
            if (mi >= mb_store) continue;                 // (wave-uniform; the tall tile's lower waves do not own their third block)
            const int m = m0 + xrow0 + 32 * mi + r;
            const bool ok = m < p.M;
            const int64_t rowoff = (int64_t)(ok ? m : 0) * p.N + nb + 8 * h;
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {
                float v[2][4];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[e][j] = acc[ni][mi][4 * (2 * qp + e) + j] + bq[2 * qp + e][j];
                const uint32_t a0 = lin_pack2<E>(v[0][0], v[0][1]), a1 = lin_pack2<E>(v[0][2], v[0][3]);
                const uint32_t b0 = lin_pack2<E>(v[1][0], v[1][1]), b1 = lin_pack2<E>(v[1][2], v[1][3]);
                const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
                if (ok) *reinterpret_cast<u32x4*>(Y + rowoff + 16 * qp) = u32x4{s0[0], s1[0], s0[1], s1[1]};
            }
        }
    }
}

template <class TR>
__global__ __launch_bounds__(512, 2) void lin128_kernel(Lin128Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int l = xcd_remap(blockIdx.x, gridDim.x);                 // an XCD's workgroups are consecutive: they share x row panels in its L2
    const int tn = l % p.tiles_n, tm = l / p.tiles_n;
    if (p.tall && tm == p.tiles_m - 1) lin128_tile<TR, 3>(p, smem, tm, tn);      // (workgroup-uniform)
    else lin128_tile<TR, 2>(p, smem, tm, tn);
}

// 16-bit matrix transpose (weights: [R, C] -> [C, R]), 64 x 64 tiles through LDS
template <class E>
__global__ __launch_bounds__(256) void transpose16_kernel(const E* __restrict__ in, E* __restrict__ out, int R, int C) {
    __shared__ E tile[64][66];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4)
        if (r0 + i < R && c0 + tx < C) tile[i][tx] = in[(int64_t)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 64; i += 4)
        if (c0 + i < C && r0 + tx < R) out[(int64_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

// Up to four 16-bit transposes [R, C] -> [C, R] in ONE launch (the transposed shadow of a residual block's four Linear weights, which
// the data-gradient products read): a workgroup per 64 x 64 tile, 16 bytes per lane on the global loads AND the global stores.
// The LDS image is the TRANSPOSED tile, element (c, r) at [c][r], 64 x 64 with no padding: a lane loads 8 columns of TWO rows, packs
// the two rows' values of each column into a dword and stores 8 dwords; it then reads 16 bytes of one image row and stores them.
// Padding cannot serve both sides -- the 16-byte reads need a row pitch that is a multiple of 4 dwords, and with any such pitch the
// 8 lanes that hold the 8 column groups of one row pair store to the same bank -- so the 16-byte slots of an image row are XOR-ed
// with the row's column group instead: the 32 lanes of a ds_write_b32 group then cover 32 banks, and the 16 lanes of a
// ds_read_b128 group 64.  A side whose pointer or row pitch is not 16-byte aligned (a view at an odd element offset of the flat
// shadow), and every tile at a ragged edge, moves 2 bytes per lane through the same image.
constexpr int kTransposeGroupMax = 4;
struct TransposeGroup {
    const uint16_t* in[kTransposeGroupMax];
    uint16_t* out[kTransposeGroupMax];
    int R[kTransposeGroupMax], C[kTransposeGroupMax];
    int first[kTransposeGroupMax + 1];      // first tile of matrix g in the launch's tile order
    int count;
};

__device__ __forceinline__ int transpose_slot(int c, int r) { return c * 64 + ((((r >> 3) ^ (c >> 3)) & 7) << 3) + (r & 7); }

__global__ __launch_bounds__(256) void transpose16_group_kernel(TransposeGroup gp) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[64 * 64];
    const int w = blockIdx.x;
    int g = 0;
#pragma unroll
    for (int i = 1; i < kTransposeGroupMax; ++i)
        if (i < gp.count && w >= gp.first[i]) g = i;
    const uint16_t* __restrict__ in = gp.in[g];
    uint16_t* __restrict__ out = gp.out[g];
    const int R = gp.R[g], C = gp.C[g];
    const int tiles_c = (C + 63) >> 6, t = w - gp.first[g];
    const int r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
    const bool full = r0 + 64 <= R && c0 + 64 <= C;                                                   // (workgroup-uniform, like all below)
    const bool wide_in = full && !(reinterpret_cast<uintptr_t>(in) & 15) && !(C & 7);
    const bool wide_out = full && !(reinterpret_cast<uintptr_t>(out) & 15) && !(R & 7);
    const int tid = threadIdx.x;
    if (wide_in) {
        const int cg = tid & 7, rp = tid >> 3;              // 8 lanes x 16 bytes = the 128 bytes of a tile row; rows 2 rp and 2 rp + 1
        const uint16_t* src = in + (int64_t)(r0 + 2 * rp) * C + c0 + 8 * cg;
        const u32x4 a = *reinterpret_cast<const u32x4*>(src), b = *reinterpret_cast<const u32x4*>(src + C);
        uint32_t* image = reinterpret_cast<uint32_t*>(tile);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t lo = (j & 1) ? a[j >> 1] >> 16 : a[j >> 1] & 0xffffu;
            const uint32_t hi = (j & 1) ? b[j >> 1] & 0xffff0000u : b[j >> 1] << 16;
            image[transpose_slot(8 * cg + j, 2 * rp) >> 1] = lo | hi;
        }
    } else {
        const int tx = tid & 63, ty = tid >> 6;
        for (int i = ty; i < 64; i += 4)
            if (r0 + i < R && c0 + tx < C) tile[transpose_slot(tx, i)] = in[(int64_t)(r0 + i) * C + c0 + tx];
    }
    __syncthreads();
    if (wide_out) {
        const int rg = tid & 7;
#pragma unroll
        for (int c = tid >> 3; c < 64; c += 32)
            *reinterpret_cast<u32x4*>(out + (int64_t)(c0 + c) * R + r0 + 8 * rg) = *reinterpret_cast<const u32x4*>(tile + transpose_slot(c, 8 * rg));
    } else {
        const int tx = tid & 63, ty = tid >> 6;
        for (int i = ty; i < 64; i += 4)
            if (c0 + i < C && r0 + tx < R) out[(int64_t)(c0 + i) * R + r0 + tx] = tile[transpose_slot(i, tx)];
    }
}

}  // namespace npcd

using namespace npcd;

static int lin_cus() {
    static const int n = [] {
        int dev = 0, cu = 256;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cu = 256;
        const char* e = getenv("NPCD_LIN_GRID");          // A/B probes only
        return e ? atoi(e) : cu;
    }();
    return n;
}

template <class TR, int EPI>
static int lin_launch(const LinParams& p, hipStream_t st) {
    static DynLds lds;
    const void* k = reinterpret_cast<const void*>(lin_kernel<TR, EPI>);
    NPCD_HIP_CHECK(lds.ensure(k, kLRing));
    const int grid = p.ntiles < lin_cus() ? p.ntiles : lin_cus();
    hipLaunchKernelGGL((lin_kernel<TR, EPI>), dim3(grid), dim3(512), kLRing, st, p);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

static int lin_common(int epi, const void* x, const void* w, const void* bias, void* y, void* y2, const void* aux, float* part, int M, int N, int K,
                      int dtype, void* stream) {
    if (!x || !w || !y || M <= 0 || N <= 0 || K <= 0) return NPCD_ERR_ARG;
    if (N % 256 || (N / 256) % 4 || K % 64 || (dtype != NPCD_BF16 && dtype != NPCD_F16)) return NPCD_ERR_UNSUPPORTED;
    if ((int64_t)M * N >= (int64_t)1 << 31 || (int64_t)M * K >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    for (const void* q : {x, w, bias, (const void*)y, (const void*)y2, aux})
        if (reinterpret_cast<uintptr_t>(q) & 15) return NPCD_ERR_ARG;
    if (epi == LIN_GELU && !y2) return NPCD_ERR_ARG;
    if (epi == LIN_DGELU && (!aux || !part || bias)) return NPCD_ERR_ARG;
    LinParams p{};
    p.x = x; p.w = w; p.bias = bias; p.y = y; p.y2 = y2; p.aux = aux; p.part = part;
    p.M = M; p.N = N; p.K = K;
    p.tiles_m = (M + 255) / 256; p.tiles_n = N / 256;
    p.ntiles = p.tiles_m * p.tiles_n;
    p.full_m = p.tiles_m / 8 * 8;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define NPCD_LIN_GO(TRT)                                                          \
    switch (epi) {                                                                \
        case LIN_PLAIN: return lin_launch<TRT, LIN_PLAIN>(p, st);                 \
        case LIN_GELU: return lin_launch<TRT, LIN_GELU>(p, st);                   \
        default: return lin_launch<TRT, LIN_DGELU>(p, st);                        \
    }
    if (dtype == NPCD_BF16) { NPCD_LIN_GO(BF16) }
    NPCD_LIN_GO(F16)
#undef NPCD_LIN_GO
}

extern "C" int npcd_linear_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int dtype, void* stream) {
    return lin_common(LIN_PLAIN, x, w, bias, y, nullptr, nullptr, nullptr, M, N, K, dtype, stream);
}
extern "C" int npcd_linear_gelu_fwd(const void* x, const void* w, const void* bias, void* h, void* g, int M, int N, int K, int dtype, void* stream) {
    return lin_common(LIN_GELU, x, w, bias, h, g, nullptr, nullptr, M, N, K, dtype, stream);
}
extern "C" int npcd_linear_dgelu_rows(int M) { return M <= 0 ? -1 : 2 * ((M + 255) / 256); }
extern "C" int npcd_linear_dgelu_bwd(const void* dy, const void* wt, const void* h, void* dh, float* part, int M, int N, int K, int dtype,
                                     void* stream) {
    return lin_common(LIN_DGELU, dy, wt, nullptr, dh, nullptr, h, part, M, N, K, dtype, stream);
}
extern "C" int npcd_linear128_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int dtype, void* stream) {
    if (!x || !w || !y || M <= 0 || N <= 0 || K <= 0) return NPCD_ERR_ARG;
    if (N % 128 || K % 64 || (dtype != NPCD_BF16 && dtype != NPCD_F16)) return NPCD_ERR_UNSUPPORTED;
    // (operands are addressed through 32-bit byte offsets of a buffer resource: below 2 GB each)
    if ((int64_t)M * N >= (int64_t)1 << 31 || (int64_t)M * K >= (int64_t)1 << 30 || (int64_t)N * K >= (int64_t)1 << 30) return NPCD_ERR_UNSUPPORTED;
    for (const void* q : {x, w, bias, (const void*)y})
        if (reinterpret_cast<uintptr_t>(q) & 15) return NPCD_ERR_ARG;
    Lin128Params p{};
    p.x = x; p.w = w; p.bias = bias; p.y = y;
    p.M = M; p.N = N; p.K = K;
    const int rem = M % 128;
    p.tall = (M > 128 && rem >= 1 && rem <= 32) ? 128 + rem : 0;       // the left-over rows ride on the last full row tile
    p.tiles_m = p.tall ? M / 128 : (M + 127) / 128;
    p.tiles_n = N / 128;
    hipStream_t st = static_cast<hipStream_t>(stream);
    static DynLds lds_b, lds_h;
    const int grid = p.tiles_m * p.tiles_n;
    if (dtype == NPCD_BF16) {
        NPCD_HIP_CHECK(lds_b.ensure(reinterpret_cast<const void*>(lin128_kernel<BF16>), kL128Lds));
        hipLaunchKernelGGL(lin128_kernel<BF16>, dim3(grid), dim3(512), kL128Lds, st, p);
    } else {
        NPCD_HIP_CHECK(lds_h.ensure(reinterpret_cast<const void*>(lin128_kernel<F16>), kL128Lds));
        hipLaunchKernelGGL(lin128_kernel<F16>, dim3(grid), dim3(512), kL128Lds, st, p);
    }
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
#ifdef NPCD_L128_TL
extern "C" int npcd_lin128_debug_read(long long* out, int count) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(npcd::g_l128_tl), sizeof(long long) * count);
}
#endif
#ifdef NPCD_LIN_TL
extern "C" int npcd_lin_debug_read(long long* out, int count) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(npcd::g_lin_tl), sizeof(long long) * count);
}
#endif
extern "C" int npcd_transpose_16(const void* in, void* out, int R, int C, void* stream) {
    if (!in || !out || R <= 0 || C <= 0) return NPCD_ERR_ARG;
    hipLaunchKernelGGL(transpose16_kernel<uint16_t>, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t*>(in), static_cast<uint16_t*>(out), R, C);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
extern "C" int npcd_transpose16_group(int count, const void* const* in, void* const* out, const int* R, const int* C, void* stream) {
    if (count < 1 || count > kTransposeGroupMax || !in || !out || !R || !C) return NPCD_ERR_ARG;
    TransposeGroup gp{};
    gp.count = count;
    int64_t tiles = 0;
    for (int g = 0; g < count; ++g) {
        if (!in[g] || !out[g] || R[g] <= 0 || C[g] <= 0) return NPCD_ERR_ARG;
        if ((reinterpret_cast<uintptr_t>(in[g]) & 1) || (reinterpret_cast<uintptr_t>(out[g]) & 1)) return NPCD_ERR_ARG;
        gp.in[g] = static_cast<const uint16_t*>(in[g]); gp.out[g] = static_cast<uint16_t*>(out[g]); gp.R[g] = R[g]; gp.C[g] = C[g];
        gp.first[g] = (int)tiles;
        tiles += (int64_t)((R[g] + 63) / 64) * ((C[g] + 63) / 64);
        if (tiles >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    }
    gp.first[count] = (int)tiles;
    hipLaunchKernelGGL(transpose16_group_kernel, dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(stream), gp);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
