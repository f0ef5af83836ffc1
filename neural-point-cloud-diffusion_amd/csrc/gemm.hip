// Weight-gradient GEMM of the denoiser's Linear layers for gfx950:  dW[N, K] (fp32) = dy[T, N]^T x[T, K],  16-bit operands.
//
// Reference: the nn.Linear weight gradients of transformer.py:67-72 (c_qkv), :107-115 (attn.c_proj), :118-137 (mlp.c_fc / c_proj),
// produced by autograd in the reference; here called from the hand-written backward of the fused backbone
// (npcd/models/diffusion/fused.py).  24 layers x 4 Linears x 2 T N K FLOP = 19.8 TFLOP of the 64.5 TFLOP step.
//
// Why an own kernel: the product reduces over the TOKEN dimension (T = 32,832 at cfg-D) into a small output (1-4 M elements =
// 16-64 tiles of 256 x 256 for 256 CUs), both operands have the reduction index as their SLOW index, and the result must be fp32.
// The library runs this at 0.74-0.98 PF/s (row-split batched GEMM + a sum pass; its fp32-output kernels are outside TunableOp).
//
// What bounded the split-T form in round 6 (measured, tools/probes/gpu_dev_wgrad_own.py + timing-only builds without the DMA / the
// matrix instructions / the reads, c_fc shape, T = 32,832; those switches left the file with the tile body they were written for):
// a 256 x 256 tile streams 128 FLOP per byte through LDS whatever the split, i.e. 2.15 GB per call; the LDS-DMA stream ALONE (no
// fragment reads, no matrix instructions) takes 170-190 us = 49 GB/s per CU, which is what 63 % L2 hits (70 GB/s per CU) and 37 %
// misses to the Infinity Cache / HBM (30 GB/s) give (rocprofv3: TCP_TCC_READ_REQ 2.15 GB, FETCH_SIZE x 2 = 788 MB -- the minimum for
// eight private L2s: every XCD needs its share of dy once and all of x).  The matrix instructions alone take ~190 us; the two overlap
// to 255-275 us -- which is also where the library is (MT256x256x32 / 256x192x64 kernels + a sum pass: 0.92-1.0 PF/s).  The kernel is
// at parity with the library, not ahead; it is an opt-in (NPCD_OWN_WGRAD=1) that makes the weight gradients bitwise reproducible
// without a library dependency.
//
// Round 18, the unsliced form on the full chip (wgrad_group_kernel with 16 products, tools/probes/gpu_dev_wgrad_multiblock.py): the
// four products of FOUR blocks are 768 tiles = three rounds of 256 CUs, one workgroup per tile over all 32,832 tokens (1,026 ring
// stages), no slabs and no sum pass.  Measured on cold, rotating operands: 2.83 ms per launch = 707 us per block (1.17 PF/s) against
// 870 us for the library's sliced products + slab sums and 841 us for one 192-tile launch per block; inside the training step the
// launch averages 3.09 ms = 773 us per block against 874 us (docs/experiments.md R18.1).  That is the default of the fused backbone
// from 20,000 token rows on.
//
// Round 21, the tile body re-pipelined (tools/probes/gpu_dev_wgrad_pipeline.py, docs/experiments.md R21.1).  Timing-only builds of
// the round-18 body in the 768-tile launch: matrix instructions + reads + barriers WITHOUT the in-loop DMA 667 us per block, DMA +
// reads without matrix instructions 516 us, the DMA stream with its waits and barriers alone 440 us, everything 759 us (826 GFLOP
// are 330 us at the 2.5 PF/s peak): the unsliced form is NOT bound by the L2 -> LDS stream; its loop lost 40 % of the matrix pipe
// with no DMA in it at all -- a barrier and two full lgkmcnt(0) drains per 32 tokens, all eight waves in lockstep, every burst of 12
// fragment reads issued with the pipe idle.  The body below runs 64 tokens per barrier and issues the reads of the next 16-token group
// between the pairs of matrix instructions of the current one, each pair behind a counted lgkmcnt: 697 against 771 us per block
// (1.19 against 1.07 PF/s, same box, alternating), every output bit the same.  Either half alone is slower than the round-18 body
// (64 tokens per barrier with burst reads 790 against 759 us; interleaved reads on 32-token steps 775 against 759 us), s_setprio
// around the pairs costs 5 % (773 against 733 us).  What bounds it now: still the issue stream of the loop rather than a unit -- the
// DMA stream alone and the matrix instructions alone are each far shorter than the launch (R21.1 has the counters of both bodies).
//
// Structure:
//   * workgroup = 8 waves = one 256 x 256 output tile over ONE slice of the token range (split-T: tiles x slices ~ 256 workgroups,
//     one per CU); every slice writes its own fp32 slab, npcd_wgrad_reduce adds the slabs in slice order (bitwise reproducible, no
//     atomics);
//   * both operands stream as [32 tokens][64 columns] sub-tiles (128-byte rows, the XOR-swizzled image of the attention kernels)
//     through a five-stage LDS ring (the CU's 160 KiB) by LDS-DMA: a step of 64 tokens = two stages is read while up to three stages
//     are in flight, one counted vmcnt and one barrier per step (the counts are argued in wgrad_tile); BOTH MFMA operands are transposed
//     reads (ds_read_b64_tr_b16) of those row-major images -- the contraction order is the same permutation of the 16 token rows for A
//     and B, so it drops out;
//   * wave = 128 (N) x 64 (K) of the tile: 8 accumulators of 32 x 32, v_mfma_f32_32x32x16, two fragment sets: the 12 reads of the
//     next 16-token group go out between the four pairs of matrix instructions of the current one (wgrad_group16); every accumulator
//     takes its 16-token groups in ascending token order, so the bits do not depend on the pipeline;
//   * workgroup -> (tile, slice) mapping keeps the workgroups that read the same dy panel on one XCD (its L2 then serves the
//     panel to all of them; x is small enough for the Infinity Cache).
#include <type_traits>

#include "common.h"

namespace npcd {

typedef __attribute__((address_space(3))) void lptr_g;

__device__ __forceinline__ uint32_t g_lds_addr(const unsigned char* p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char*)p;
}
__device__ __forceinline__ const void* g_uniform_ptr(const void* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const void*>(((uint64_t)hi << 32) | lo);
}
// one LDS-DMA wave-instruction: wave-uniform 64-bit base + one 32-bit byte offset per lane -> LDS (M0 = wave-uniform destination)
__device__ __forceinline__ void g_dma16(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    sbase = g_uniform_ptr(sbase);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
template <int OFF>
__device__ __forceinline__ u32x2 g_tr(uint32_t addr) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
struct GFrag {
    u32x2 lo, hi;
};
template <class TR>
__device__ __forceinline__ typename TR::vec8 g_vec(const GFrag& t) {
    const u32x4 x = {t.lo[0], t.lo[1], t.hi[0], t.hi[1]};
    return __builtin_bit_cast(typename TR::vec8, x);
}

struct WgradParams {
    const void* dy;   // [T, N]
    const void* x;    // [T, K]
    float* out;       // [S][N][K] slabs (S == 1: the result itself)
    int T, N, K, S;
    int tiles_n, tiles_k;
};
constexpr int kStage = 32768;          // one ring stage = 32 tokens: 4 dy sub-tiles + 4 x sub-tiles of [32 tokens][64 columns] = 4 KiB each
constexpr int kSub = 4096;
constexpr int kRing = 5;               // stages = the CU's 160 KiB: the two of the 64-token step being read, up to three in flight
constexpr uint32_t kRingBytes = kRing * kStage;

// where a wave's share of a stage's DMA comes from: sub-tile `wave` (waves 0..3: dy columns n0 + 64 wave; waves 4..7: x columns
// k0 + 64 (wave - 4)); rows from T on come from a page of zeros
template <class E>
struct DmaSrc {
    const E* base;
    const E* zeros;
    int64_t ld;
    int col0, lane, T;
};

// piece i (8 rows x 128 B) of the [32 token][64 column] sub-tile that starts at token t0: one DMA wave-instruction
template <class E>
__device__ __forceinline__ void dma_piece(const DmaSrc<E>& d, int i, uint32_t lds_dst, int t0) {
    const int rowin = d.lane >> 3, prow = i * 8 + rowin;
    const int chunk = (d.lane & 7) ^ tile_swz(prow);
    if (t0 + i * 8 + 8 <= d.T) {                                    // (wave-uniform) all eight rows exist
        const char* sb = reinterpret_cast<const char*>(d.base + (int64_t)(t0 + i * 8) * d.ld + d.col0);
        g_dma16(sb, (uint32_t)((rowin * d.ld + chunk * 8) * (int64_t)sizeof(E)), __builtin_amdgcn_readfirstlane(lds_dst + i * 1024));
    } else {
        // the ragged end of the token range: per-lane choice between the row and the zero page (64-bit per-lane address form)
        const E* src = (t0 + prow < d.T) ? d.base + (int64_t)(t0 + prow) * d.ld + d.col0 + chunk * 8 : d.zeros + (d.lane & 7) * 8;
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_dst + i * 1024)) : "memory");
    }
}
template <class E>
__device__ __forceinline__ void dma_subtile(const DmaSrc<E>& d, uint32_t lds_dst, int t0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_piece<E>(d, i, lds_dst, t0);
}

__device__ unsigned char g_zero_page[128];      // (zero-initialised device memory)

// The 12 transposed reads of one 16-token group (G16 = 0 / 1: token rows [0, 16) / [16, 32) of a stage) go out in the order the matrix
// instructions take them -- the two B fragments, then A[0..3] -- so that a counted lgkmcnt can release each pair of matrix
// instructions as soon as its own operands are there.  ta / tb: the lane's four fragment addresses inside the stage's first dy / its x
// sub-tile.
template <int G16>
__device__ __forceinline__ void rd_b(GFrag (&fb)[2], const uint32_t (&tb)[2][2]) {
    fb[0].lo = g_tr<G16 * 2048>(tb[0][0]); fb[0].hi = g_tr<G16 * 2048>(tb[0][1]);
    fb[1].lo = g_tr<G16 * 2048>(tb[1][0]); fb[1].hi = g_tr<G16 * 2048>(tb[1][1]);
}
template <int G16, int M>
__device__ __forceinline__ void rd_a(GFrag (&fa)[4], const uint32_t (&ta)[2][2]) {
    fa[M].lo = g_tr<(M >> 1) * kSub + G16 * 2048>(ta[M & 1][0]);
    fa[M].hi = g_tr<(M >> 1) * kSub + G16 * 2048>(ta[M & 1][1]);
}
#define NPCD_G_LGKM(N)                                           \
    do {                                                         \
        asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory"); \
        __builtin_amdgcn_sched_barrier(0);                       \
    } while (0)
// Rows 32 M .. 32 M + 31 of the wave's tile take one 16-token group: two matrix instructions, behind a wait for at most WAIT outstanding
// LDS operations (WAIT < 0: none).  A matrix instruction touches no memory, so neither a memory clobber nor the order of the source
// keeps it behind the wait that covers its operands; what does is a data dependence: the wait (an asm volatile statement, ordered with
// every read and every other wait) takes the two accumulators as read-write operands, and so does an empty statement behind the pair,
// which keeps the pair in front of the reads that follow it in the source.
template <class TR, int M, int WAIT>
__device__ __forceinline__ void mma_pair(f32x16 (&acc)[4][2], const GFrag (&ca)[4], const GFrag (&cb)[2]) {
    if (WAIT >= 0) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(acc[M][0]), "+v"(acc[M][1]) : "n"(WAIT < 0 ? 0 : WAIT) : "memory");
    else asm volatile("" : "+v"(acc[M][0]), "+v"(acc[M][1]));
    acc[M][0] = TR::mfma32(g_vec<TR>(ca[M]), g_vec<TR>(cb[0]), acc[M][0]);
    acc[M][1] = TR::mfma32(g_vec<TR>(ca[M]), g_vec<TR>(cb[1]), acc[M][1]);
    asm volatile("" : "+v"(acc[M][0]), "+v"(acc[M][1]));
}
// One 16-token group of the wave: its 8 matrix instructions from (ca, cb) while the 12 reads of the NEXT group (half G16N of the stage
// ta / tb point into) go out into (na, nb) between the pairs, and -- DMA, when `dma` -- the four pieces of one stage's sub-tile.
// OWN: the 12 reads of (ca, cb) are the youngest LDS operations of the wave and may all be outstanding on entry; each pair then waits
// for its own operands only: outstanding <= (own reads behind the ones it needs) + (reads of the next group issued so far).  Not OWN:
// the caller has waited lgkmcnt(0).  The waits are correct because LDS operations return in issue order and every one of them in this
// loop is an asm volatile statement (issue order = source order); mma_pair ties each pair to its wait.
template <class TR, int G16N, bool OWN, bool DMA, class E>
__device__ __forceinline__ void wgrad_group16(f32x16 (&acc)[4][2], const GFrag (&ca)[4], const GFrag (&cb)[2], GFrag (&na)[4], GFrag (&nb)[2],
                                              const uint32_t (&ta)[2][2], const uint32_t (&tb)[2][2], const DmaSrc<E>& d, bool dma,
                                              uint32_t dma_dst, int dma_t0) {
    mma_pair<TR, 0, OWN ? 6 : -1>(acc, ca, cb);       // B[0], B[1], A[0] of this group: the first 6 of its 12
    rd_b<G16N>(nb, tb);                               // + 4 of the next group
    if (DMA && dma) dma_piece<E>(d, 0, dma_dst, dma_t0);
    mma_pair<TR, 1, OWN ? 8 : -1>(acc, ca, cb);       // A[1]: behind it A[2], A[3] (4) + 4
    rd_a<G16N, 0>(na, ta); rd_a<G16N, 1>(na, ta);
    if (DMA && dma) dma_piece<E>(d, 1, dma_dst, dma_t0);
    mma_pair<TR, 2, OWN ? 10 : -1>(acc, ca, cb);      // A[2]: behind it A[3] (2) + 8
    rd_a<G16N, 2>(na, ta); rd_a<G16N, 3>(na, ta);
    if (DMA && dma) dma_piece<E>(d, 2, dma_dst, dma_t0);
    mma_pair<TR, 3, OWN ? 12 : -1>(acc, ca, cb);      // A[3]: behind it the 12 of the next group
    if (DMA && dma) dma_piece<E>(d, 3, dma_dst, dma_t0);
}

// one 256 x 256 output tile at (n0, k0) over the ring stages [s_lo, s_hi) of the token range, written to `out` (row pitch p.K)
template <class TR>
__device__ __forceinline__ void wgrad_tile(const WgradParams& p, float* out, int n0, int k0, int s_lo, int s_hi) {
    using E = typename TR::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // kRing stages x 32 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;                                   // wave tile: rows [128 wm, +128) x columns [64 wn, +64)
    const uint32_t lds0 = g_lds_addr(smem);
    // 64-token steps: an odd number of stages is padded with one stage of zeros (rows from s_hi * 32 on read the zero page like the
    // rows from T on; a matrix instruction on zero operands leaves its accumulator as it is)
    const int nsteps = (s_hi - s_lo + 1) >> 1, n2 = 2 * nsteps;
    const bool isx = wave >= 4;
    DmaSrc<E> d;
    d.base = isx ? static_cast<const E*>(p.x) : static_cast<const E*>(p.dy);
    d.zeros = reinterpret_cast<const E*>(g_zero_page);
    d.ld = isx ? p.K : p.N;
    d.col0 = isx ? k0 + 64 * (wave - 4) : n0 + 64 * wave;
    d.lane = lane;
    d.T = p.T < s_hi * 32 ? p.T : s_hi * 32;
    const uint32_t ddst = lds0 + wave * kSub;

    // fragment addresses inside a sub-tile (sub-tile / 16-row step go into immediates, the stage into one add)
    uint32_t tr[2][2];
    {
        const int grp = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3, h = grp >> 1;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const int col = db * 32 + 16 * (grp & 1) + 4 * pp;
#pragma unroll
            for (int hi = 0; hi < 2; ++hi) tr[db][hi] = lds0 + tile_off(4 * h + q + 8 * hi, col >> 3) + (col & 7) * 2;
        }
    }
    const uint32_t a_off = (2 * wm) * kSub, b_off = (4 + wn) * kSub;
    uint32_t ta[2][2], tb[2][2];
#define NPCD_G_ADDR(SO)                                       \
    do {                                                      \
        _Pragma("unroll") for (int db = 0; db < 2; ++db)      \
            _Pragma("unroll") for (int hi = 0; hi < 2; ++hi) { \
                ta[db][hi] = tr[db][hi] + ((SO) + a_off);     \
                tb[db][hi] = tr[db][hi] + ((SO) + b_off);     \
            }                                                 \
    } while (0)

    f32x16 acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x16{0};

    // Ring protocol.  Stage q (32 tokens) lives in slot q mod 5; step j (64 tokens) reads stages 2 j and 2 j + 1 and ends with the one
    // barrier B_j of the step; the last 16-token group of step j runs BEHIND B_j (from registers) while the first reads of step j + 1 go
    // out.  A wave issues 4 DMA instructions per stage, and VMEM operations retire in issue order:
    //   issue order   prologue: stages 0, 1, 2, 3.  Step j issues stage 2 j + 4 in its first group and stage 2 j + 5 in its last, behind
    //                 B_j: in front of B_j the youngest stage out is 2 j + 4, and 2 j + 3 went out behind B_(j-1) (or in the prologue).
    //   RAW           before B_j a wave waits vmcnt(4): at most the 4 instructions of stage 2 j + 4, the youngest, are outstanding, so
    //                 its share of stages 2 j + 2 and 2 j + 3 has landed (vmcnt(0) when stage 2 j + 4 does not exist); every wave has
    //                 done so when B_j releases, and stages 2 j + 2 / 2 j + 3 are read only behind B_j.  Prologue: vmcnt(8) leaves
    //                 stages 2 and 3 outstanding, stages 0 and 1 are read behind its barrier.
    //   WAR           stage 2 j + 4 goes to the slot of stage 2 j - 1 and is issued behind B_(j-1); stage 2 j + 5 goes to the slot of
    //                 stage 2 j and is issued behind B_j.  Every read of stages 2 j and 2 j + 1 is issued before B_j and retired by
    //                 the lgkmcnt(0) in front of it, by every wave.  (Slots 3 and 4 are first filled by stages 3 and 4: nothing to wait for.)
    //   in flight     behind step j's first group: stages 2 j + 2, 2 j + 3, 2 j + 4 -- three, as with the four-stage ring of 32-token
    //                 steps; a stage is issued at least one step (two stage times) before the wait that needs it.
#define NPCD_G_VMWAIT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
    if (nsteps > 0) {
        // prologue: stages 0 .. 3 into slots 0 .. 3 (nothing has read them); stages 0 and 1 have landed when at most the 8
        // instructions of stages 2 and 3 are outstanding
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < n2) dma_subtile<E>(d, ddst + q * kStage, (s_lo + q) * 32);
        if (n2 > 2) NPCD_G_VMWAIT(8);
        else NPCD_G_VMWAIT(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    GFrag fa0[4] = {}, fb0[2] = {}, fa1[4] = {}, fb1[2] = {};
    uint32_t r0 = 0;                                     // byte offset of the slot of stage 2 j
    NPCD_G_ADDR(r0);
    if (nsteps > 0) {
        rd_b<0>(fb0, tb);
        rd_a<0, 0>(fa0, ta); rd_a<0, 1>(fa0, ta); rd_a<0, 2>(fa0, ta); rd_a<0, 3>(fa0, ta);
    }
    for (int j = 0; j < nsteps; ++j) {
        uint32_t r1 = r0 + kStage; r1 = r1 >= kRingBytes ? r1 - kRingBytes : r1;
        uint32_t r2 = r1 + kStage; r2 = r2 >= kRingBytes ? r2 - kRingBytes : r2;
        uint32_t r4 = r2 + 2 * kStage; r4 = r4 >= kRingBytes ? r4 - kRingBytes : r4;
        const bool more = 2 * j + 4 < n2;                // stages 2 j + 4 and 2 j + 5 exist (n2 is even)
        const int t4 = (s_lo + 2 * j + 4) * 32;
        // tokens [0, 16) of stage 2 j; reads: [16, 32) of stage 2 j; DMA: stage 2 j + 4 -> the slot of stage 2 j - 1
        wgrad_group16<TR, 1, true, true, E>(acc, fa0, fb0, fa1, fb1, ta, tb, d, more, ddst + r4, t4);
        NPCD_G_ADDR(r1);
        // tokens [16, 32) of stage 2 j; reads: [0, 16) of stage 2 j + 1
        wgrad_group16<TR, 0, true, false, E>(acc, fa1, fb1, fa0, fb0, ta, tb, d, false, 0u, 0);
        // tokens [0, 16) of stage 2 j + 1; reads: [16, 32) of stage 2 j + 1
        wgrad_group16<TR, 1, true, false, E>(acc, fa0, fb0, fa1, fb1, ta, tb, d, false, 0u, 0);
        NPCD_G_ADDR(r2);
        // this wave has read everything it needs of stages 2 j and 2 j + 1; its share of stages 2 j + 2 and 2 j + 3 has landed when at
        // most the 4 instructions of stage 2 j + 4 are outstanding
        NPCD_G_LGKM(0);
        if (more) NPCD_G_VMWAIT(4);
        else NPCD_G_VMWAIT(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // tokens [16, 32) of stage 2 j + 1; reads: [0, 16) of stage 2 j + 2 (past the last step: of a slot nobody waits for; the
        // values are not used); DMA: stage 2 j + 5 -> the slot of stage 2 j
        wgrad_group16<TR, 0, false, true, E>(acc, fa1, fb1, fa0, fb0, ta, tb, d, more, ddst + r0, t4 + 32);
        r0 = r2;
    }
    NPCD_G_LGKM(0);
#undef NPCD_G_ADDR
#undef NPCD_G_VMWAIT
    // ---- row n0 + 128 wm + 32 mi + acc_row(i, hh), column k0 + 64 wn + 32 ni + (lane & 31)
    const int r = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            float* o = out + (int64_t)(n0 + 128 * wm + 32 * mi) * p.K + k0 + 64 * wn + 32 * ni + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[(int64_t)acc_row(i, hh) * p.K] = acc[mi][ni][i];
        }
}
#undef NPCD_G_LGKM

template <class TR>
__global__ __launch_bounds__(512, 2) void wgrad_kernel(WgradParams p) {
    // workgroup -> (n tile, slice, k tile): k fastest, so that the workgroups of one XCD chunk share dy panels
    const int w = xcd_remap(blockIdx.x, gridDim.x);
    const int tk = w % p.tiles_k, s = (w / p.tiles_k) % p.S, tn = w / (p.tiles_k * p.S);
    const int steps = (p.T + 31) >> 5;                                         // ring stages of 32 tokens
    const int s_lo = (int)((int64_t)steps * s / p.S), s_hi = (int)((int64_t)steps * (s + 1) / p.S);
    wgrad_tile<TR>(p, p.out + (int64_t)s * p.N * p.K, tn * 256, tk * 256, s_lo, s_hi);      // the slab of this slice
}

// Several weight gradients over the SAME token range in one launch (the four Linear layers of a residual block at the token count of
// one rank of the 8-GPU job): every 256 x 256 output tile of every product is ONE workgroup over the whole token range -- no slices,
// no slabs, no second kernel, one fixed summation order per element.  4,104 tokens x (3072 + 1024 + 4096 + 1024) x 1024: 192 tiles,
// i.e. one round on 192 of the 256 CUs; the launch runs on a side stream beside the backward's critical path, which takes the rest.
// Up to 16 products: at the token count of a whole batch (T = 32,832) the four products of FOUR blocks are 768 tiles = three full
// rounds of 256 CUs in one launch on the main stream (npcd_wgrad_group_blocks says how many blocks fill the chip).  The tile order is
// product-major with k fastest inside a product, so the contiguous run of tiles xcd_remap hands an XCD shares dy panels and x.
constexpr int kWgradGroupMax = 16;
struct WgradGroup {
    const void* dy[kWgradGroupMax];
    const void* x[kWgradGroupMax];
    float* out[kWgradGroupMax];
    int N[kWgradGroupMax], K[kWgradGroupMax];
    int first[kWgradGroupMax + 1];      // first tile of product g in the launch's tile order
    int T, count;
};

template <class TR>
__global__ __launch_bounds__(512, 2) void wgrad_group_kernel(WgradGroup gp) {
    const int w = xcd_remap(blockIdx.x, gridDim.x);
    int g = 0;
#pragma unroll
    for (int i = 1; i < kWgradGroupMax; ++i)
        if (i < gp.count && w >= gp.first[i]) g = i;
    WgradParams p;
    p.dy = gp.dy[g]; p.x = gp.x[g]; p.out = gp.out[g];
    p.T = gp.T; p.N = gp.N[g]; p.K = gp.K[g]; p.S = 1;
    p.tiles_n = p.N / 256; p.tiles_k = p.K / 256;
    const int t = w - gp.first[g];
    wgrad_tile<TR>(p, p.out, (t / p.tiles_k) * 256, (t % p.tiles_k) * 256, 0, (gp.T + 31) >> 5);
}

// out[i] = slab[0][i] + slab[1][i] + ... in slice order (fp32, 16 bytes per thread and trip)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const f32x4* __restrict__ slabs, f32x4* __restrict__ out, int S, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 a = __builtin_nontemporal_load(slabs + i);
        for (int s = 1; s < S; ++s) a += __builtin_nontemporal_load(slabs + s * n4 + i);
        out[i] = a;
    }
}

}  // namespace npcd

using namespace npcd;

static int wgrad_slices(int T, int N, int K) {
    const int tiles = (N / 256) * (K / 256);
    static const int forced = [] { const char* e = getenv("NPCD_WGRAD_SLICES"); return e ? atoi(e) : 0; }();     // A/B probes only
    int S = forced > 0 ? forced : 256 / tiles;
    const int steps = (T + 31) / 32;
    if (S > steps / 16) S = steps / 16;        // at least 16 ring stages (512 tokens) per slice
    if (S > 16) S = 16;
    return S < 1 ? 1 : S;
}

extern "C" int npcd_wgrad_slices(int T, int N, int K) {
    if (T <= 0 || N <= 0 || K <= 0 || N % 256 || K % 256) return -1;
    return wgrad_slices(T, N, K);
}

// dW [N, K] fp32 = dy[T, N]^T x[T, K].  workspace: npcd_wgrad_slices(T, N, K) slabs of N K floats (unused when that is 1).
extern "C" int npcd_wgrad(const void* dy, const void* x, float* out, float* workspace, int T, int N, int K, int dtype, void* stream) {
    if (!dy || !x || !out || T <= 0 || N <= 0 || K <= 0) return NPCD_ERR_ARG;
    if (N % 256 || K % 256 || (dtype != NPCD_BF16 && dtype != NPCD_F16)) return NPCD_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(dy) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return NPCD_ERR_ARG;
    const int S = wgrad_slices(T, N, K);
    if (S > 1 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15))) return NPCD_ERR_ARG;
    WgradParams p{};
    p.dy = dy; p.x = x; p.out = S > 1 ? workspace : out;
    p.T = T; p.N = N; p.K = K; p.S = S;
    p.tiles_n = N / 256; p.tiles_k = K / 256;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = p.tiles_n * p.tiles_k * S;
    static DynLds lds_b, lds_h;
    if (dtype == NPCD_BF16) {
        NPCD_HIP_CHECK(lds_b.ensure(reinterpret_cast<const void*>(wgrad_kernel<BF16>), kRing * kStage));
        hipLaunchKernelGGL(wgrad_kernel<BF16>, dim3(grid), dim3(512), kRing * kStage, st, p);
    } else {
        NPCD_HIP_CHECK(lds_h.ensure(reinterpret_cast<const void*>(wgrad_kernel<F16>), kRing * kStage));
        hipLaunchKernelGGL(wgrad_kernel<F16>, dim3(grid), dim3(512), kRing * kStage, st, p);
    }
    if (S > 1) {
        const int64_t n4 = (int64_t)N * K / 4;
        const int rgrid = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rgrid), dim3(256), 0, st, reinterpret_cast<const f32x4*>(workspace), reinterpret_cast<f32x4*>(out), S, n4);
    }
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

// count (<= 16) weight gradients dW_g [N_g, K_g] fp32 = dy_g[T, N_g]^T x_g[T, K_g] over one token range in ONE launch: one workgroup per
// 256 x 256 output tile over all T tokens (no slices, no workspace); meant for token counts of a few thousand, where the tiles of all
// products together are whole rounds of the chip (npcd_wgrad_group_blocks).  Same shape rules as npcd_wgrad per product; every product
// writes its own output (two products with one `out` would be two workgroups storing to the same tile: NPCD_ERR_ARG).
extern "C" int npcd_wgrad_group(int count, const void* const* dy, const void* const* x, float* const* out, const int* N, const int* K, int T,
                                int dtype, void* stream) {
    if (count < 1 || count > kWgradGroupMax || !dy || !x || !out || !N || !K || T <= 0) return NPCD_ERR_ARG;
    if (dtype != NPCD_BF16 && dtype != NPCD_F16) return NPCD_ERR_UNSUPPORTED;
    WgradGroup gp{};
    gp.T = T; gp.count = count;
    int tiles = 0;
    for (int g = 0; g < count; ++g) {
        if (!dy[g] || !x[g] || !out[g] || N[g] <= 0 || K[g] <= 0) return NPCD_ERR_ARG;
        if (N[g] % 256 || K[g] % 256) return NPCD_ERR_UNSUPPORTED;
        if ((reinterpret_cast<uintptr_t>(dy[g]) & 15) || (reinterpret_cast<uintptr_t>(x[g]) & 15) || (reinterpret_cast<uintptr_t>(out[g]) & 15)) return NPCD_ERR_ARG;
        for (int h = 0; h < g; ++h)
            if (out[h] == out[g]) return NPCD_ERR_ARG;
        gp.dy[g] = dy[g]; gp.x[g] = x[g]; gp.out[g] = out[g]; gp.N[g] = N[g]; gp.K[g] = K[g];
        gp.first[g] = tiles;
        tiles += (N[g] / 256) * (K[g] / 256);
    }
    gp.first[count] = tiles;
    hipStream_t st = static_cast<hipStream_t>(stream);
    static DynLds lds_b, lds_h;
    if (dtype == NPCD_BF16) {
        NPCD_HIP_CHECK(lds_b.ensure(reinterpret_cast<const void*>(wgrad_group_kernel<BF16>), kRing * kStage));
        hipLaunchKernelGGL(wgrad_group_kernel<BF16>, dim3(tiles), dim3(512), kRing * kStage, st, gp);
    } else {
        NPCD_HIP_CHECK(lds_h.ensure(reinterpret_cast<const void*>(wgrad_group_kernel<F16>), kRing * kStage));
        hipLaunchKernelGGL(wgrad_group_kernel<F16>, dim3(tiles), dim3(512), kRing * kStage, st, gp);
    }
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

// How many residual blocks to put into one npcd_wgrad_group launch: the smallest G >= 1 with G * products_per_block <= max_products
// whose G * tiles_per_block workgroups (one per 256 x 256 tile, one per CU at a time) fill whole rounds of the device's CUs to at
// least 0.95; 0 when no G does (the caller keeps its per-product path).  Width 1,024: 192 tiles per block -> 4 on 256 CUs (768 tiles,
// three full rounds); width 2,048: 768 tiles -> 1.
static int wgrad_group_blocks_rule(int tiles_per_block, int max_products, int products_per_block, int cus) {
    if (tiles_per_block <= 0 || products_per_block <= 0 || cus <= 0) return 0;
    for (int G = 1; G * products_per_block <= max_products; ++G) {
        const int64_t tiles = (int64_t)G * tiles_per_block, rounds = (tiles + cus - 1) / cus;
        if (tiles * 100 >= rounds * cus * 95) return G;
    }
    return 0;
}

extern "C" int npcd_wgrad_group_blocks(int tiles_per_block, int max_products, int products_per_block) {
    if (max_products > kWgradGroupMax) max_products = kWgradGroupMax;
    int dev = 0, cus = 0;                                      // (the current device's: asked every time, the caller caches per shape)
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return wgrad_group_blocks_rule(tiles_per_block, max_products, products_per_block, cus);
}
