// The edges of one triangle mesh and Taubin smoothing on an integer lattice.  The per-lane arithmetic is csrc/smooth.h,
// shared with the host program csrc/smooth_host.cpp; this file is the launches around it.  Compiled without FMA contraction (build.py).
//
//   npcd_mesh_edges_keys, one launch: one lane per face writes its six sort keys.
//   npcd_mesh_edges_unique, one memset and two launches over the caller's ascending order of those keys:
//     marks       one lane per position: 1 for a head, 2^32 more for a head with a < b; the inclusive sums of both inside a strip of
//                 kSmStrip positions (block_scan of csrc/block_scan.h) to the workspace, the strip's total to its slot; the
//                 last valid position writes F_v to counts[1].
//     totals      one workgroup: the exclusive sums of the strip totals in place (block_scan_totals); D to counts[0].
//   npcd_mesh_edges_emit, one memset and two launches:
//     emit        one lane per position, sm_emit_lane; the four counts of a strip are summed in one 64-bit word (the scan's total)
//                 and stored to the strip's slot.
//     counts      one workgroup sums the slots and writes the four sums to counts[2..5].  No atomics: ~100,000 waves adding to one
//                 address took 1.1 ms of a 1.9-ms call on a mesh of a million faces (docs/experiments.md R34.1).
//   npcd_smooth_mesh, one memset and 3 + steps launches:
//     measure     the integer maximum of the bits of the finite |coordinates| (wave_publish_max of csrc/wave.h).
//     quantise    one lane per vertex: its record (place on the lattice, lost, moves).
//     step        one lane per vertex gathers the records of its row and writes its new record to the other buffer: no atomics.
//     finish      one lane per vertex: fp32 of its place, or its input bits.
//   Integer maxima and sums throughout: no result depends on the order of an atomic or a scan, and no workgroup waits on another --
//   the launches are the only ordering.  Every store is an ordinary vector store.
//
// Bounds.  A lane past the last face, position or vertex reads and writes nothing (it scans 0).  An index of a face outside [0, V)
// makes no key; a key's ends are below V and a rank below D before anything is written through them (sm_emit_lane); a row's ends are
// held to [0, D] and a neighbour to [0, V) before the state is read through them (sm_row, sm_step_lane).
#include "block_scan.h"
#include "common.h"
#include "smooth.h"

namespace npcd {

struct SmWs {          // the workspace of the edges: 8-byte aligned base
    uint64_t* strip_before;          // [strips(6F)]: heads | edges << 32 before the strip
    uint64_t* strip_counts;          // [strips(6F)]: used | boundary << 16 | non-manifold << 32 | misoriented << 48 of the strip
    uint32_t* incl;                  // [6F]: the inclusive counts inside the strip, heads | edges << 16
};
static inline int64_t sm_ws_layout(void* ws, int64_t F, SmWs* out) {
    const int64_t n = 6 * F, strips = sm_strips(n);
    out->strip_before = static_cast<uint64_t*>(ws);
    out->strip_counts = out->strip_before + strips;
    out->incl = reinterpret_cast<uint32_t*>(out->strip_counts + strips);
    return 16 * strips + 4 * n;
}

__global__ __launch_bounds__(kSmThreads) void sm_keys_kernel(const int32_t* faces, int64_t V, int64_t F, int64_t* keys) {
    const int64_t f = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
    if (f >= F) return;
    int64_t k[6];
    const int32_t face[3] = {faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2]};
    sm_face_keys(face, V, k);
    for (int j = 0; j < 6; ++j) keys[f * 6 + j] = k[j];
}

__global__ __launch_bounds__(kSmThreads) void sm_marks_kernel(const int64_t* keys, int64_t n, SmWs ws, int64_t* counts) {
    __shared__ uint64_t wave_total[kSmThreads / 64];
    const int64_t p = (int64_t)blockIdx.x * kSmStrip + threadIdx.x;
    const uint64_t own = p < n ? sm_marks(keys, p) : 0;
    uint64_t total;
    const uint64_t incl = block_scan<kSmThreads, true>(own, wave_total, &total);
    if (p < n) {
        ws.incl[p] = (uint32_t)incl | (uint32_t)(incl >> 32) << 16;
        if (sm_is_last(keys, n, p)) counts[kSmCountFaces] = (p + 1) / 6;
    }
    if (threadIdx.x == 0) ws.strip_before[blockIdx.x] = total;
}

// one workgroup: totals [n] (two 32-bit counts in a word) to their exclusive sums in place; the low count of all to *out
__global__ __launch_bounds__(kSmThreads) void sm_totals_kernel(uint64_t* totals, int64_t n, int64_t* out) {
    __shared__ uint64_t wave_total[kSmThreads / 64];
    const uint64_t sum = block_scan_totals<kSmThreads, false>(totals, n, wave_total);
    if (threadIdx.x == 0) *out = (int64_t)(sum & 0xffffffffu);
}

__global__ __launch_bounds__(kSmThreads) void sm_emit_kernel(const int64_t* keys, int64_t n, SmWs ws, SmEdges o) {
    static_assert(kSmThreads == kSmStrip, "a workgroup of the emit launch is a strip");
    __shared__ uint64_t wave_total[kSmThreads / 64];
    const int64_t p = (int64_t)blockIdx.x * kSmStrip + threadIdx.x;
    uint64_t found = 0;
    if (p < n) {
        const uint64_t before = ws.strip_before[p / kSmStrip];
        const uint32_t incl = ws.incl[p];
        found = sm_emit_lane(keys, n, p, (int64_t)(before & 0xffffffffu) + (incl & 0xffffu), (int64_t)(before >> 32) + (incl >> 16), o);
    }
    uint64_t sum;
    block_scan<kSmThreads, true>(found, wave_total, &sum);          // every lane of the workgroup is here; at most 256 to a field
    if (threadIdx.x == 0) ws.strip_counts[blockIdx.x] = sum;
}

// one workgroup: the four 16-bit counts of every strip summed to counts [4]
__global__ __launch_bounds__(kSmThreads) void sm_counts_kernel(const uint64_t* strip_counts, int64_t strips, int64_t* counts) {
    __shared__ uint64_t wave_total[kSmThreads / 64];
    uint64_t own[4] = {0, 0, 0, 0};
    for (int64_t s = threadIdx.x; s < strips; s += kSmThreads) {
        const uint64_t c = strip_counts[s];
        for (int k = 0; k < 4; ++k) own[k] += (c >> (16 * k)) & 0xffffu;
    }
    for (int k = 0; k < 4; ++k) {
        uint64_t sum;
        block_scan<kSmThreads, true>(own[k], wave_total, &sum);
        if (threadIdx.x == 0) counts[k] = (int64_t)sum;
    }
}

struct SmArgs {
    const float* vertices;
    const int32_t *row_start, *neighbours;
    const uint8_t *boundary, *fixed;
    uint32_t* a_max;
    float* out;
    int64_t V, D;
};

__global__ __launch_bounds__(kSmThreads) void sm_measure_kernel(SmArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
    uint32_t bits = 0;
    if (i < a.V)
        for (int k = 0; k < 3; ++k) {
            const uint32_t m = finite_abs_bits(a.vertices[i * 3 + k]);
            bits = m > bits ? m : bits;
        }
    wave_publish_max(bits, a.a_max);          // every lane of the wave is here
}

__global__ __launch_bounds__(kSmThreads) void sm_quantise_kernel(SmArgs a, SmRecord* state) {
    const int64_t i = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
    if (i >= a.V) return;
    state[i] = sm_quantise_lane(a.vertices, i, a.V, a.row_start, a.neighbours, a.D, a.boundary, a.fixed, *a.a_max);
}

__global__ __launch_bounds__(kSmThreads) void sm_step_kernel(SmArgs a, const SmRecord* from, SmRecord* to, double factor) {
    const int64_t i = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
    if (i >= a.V) return;
    to[i] = sm_step_lane(from, i, a.V, a.row_start, a.neighbours, a.D, factor);
}

__global__ __launch_bounds__(kSmThreads) void sm_finish_kernel(SmArgs a, const SmRecord* state) {
    const int64_t i = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
    if (i >= a.V) return;
    float out[3];
    sm_finish_lane(a.vertices + i * 3, state[i], *a.a_max, out);
    a.out[i * 3] = out[0], a.out[i * 3 + 1] = out[1], a.out[i * 3 + 2] = out[2];
}

static int sm_check(int64_t V, int64_t F) {
    if (V < 0 || F < 0) return NPCD_ERR_ARG;
    // an index is 31 bits of a key; 6F positions are counted in 32 bits, two counts to a word
    if (V >= kSmMaxVertices || F >= kSmMaxFaces) return NPCD_ERR_UNSUPPORTED;
    return NPCD_OK;
}
// the smoothing's workspace: the maximum in the first 16 bytes, then two buffers of records
static inline int64_t sm_state_bytes(int64_t V) { return 16 + 2 * V * (int64_t)sizeof(SmRecord); }

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_mesh_edges_ws_bytes(int64_t V, int64_t F) {
    const int rc = sm_check(V, F);
    if (rc != NPCD_OK) return rc;
    SmWs w;
    return sm_ws_layout(nullptr, F, &w);
}

extern "C" int npcd_mesh_edges_keys(const int32_t* faces, int64_t V, int64_t F, int64_t* keys, void* stream) {
    const int rc = sm_check(V, F);
    if (rc != NPCD_OK) return rc;
    if (F < 1 || !faces || !keys || misaligned(faces, 4) || misaligned(keys, 8)) return NPCD_ERR_ARG;
    hipLaunchKernelGGL(sm_keys_kernel, dim3(blocks_for(F, kSmThreads)), dim3(kSmThreads), 0, static_cast<hipStream_t>(stream), faces, V, F,
                       keys);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_mesh_edges_unique(const int64_t* sorted_keys, int64_t V, int64_t F, void* ws, int64_t* counts, void* stream) {
    const int rc = sm_check(V, F);
    if (rc != NPCD_OK) return rc;
    if (F < 1 || !sorted_keys || !ws || !counts) return NPCD_ERR_ARG;
    if (misaligned(sorted_keys, 8) || misaligned(ws, 8) || misaligned(counts, 8)) return NPCD_ERR_ARG;
    SmWs w;
    sm_ws_layout(ws, F, &w);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = 6 * F, strips = sm_strips(n);
    NPCD_HIP_CHECK(hipMemsetAsync(counts, 0, kSmCounts * sizeof(int64_t), s));
    hipLaunchKernelGGL(sm_marks_kernel, dim3((unsigned)strips), dim3(kSmThreads), 0, s, sorted_keys, n, w, counts);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sm_totals_kernel, dim3(1), dim3(kSmThreads), 0, s, w.strip_before, strips, counts + kSmCountD);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_mesh_edges_emit(const int64_t* sorted_keys, int64_t V, int64_t F, void* ws, int64_t D, int32_t* row_start,
                                    int32_t* neighbours, int32_t* edges, int32_t* edge_faces, int32_t* edge_forward,
                                    uint8_t* boundary_vertex, int64_t* counts, void* stream) {
    const int rc = sm_check(V, F);
    if (rc != NPCD_OK) return rc;
    if (F < 1 || V < 1 || D < 2 || D > 6 * F || (D & 1)) return NPCD_ERR_ARG;
    if (!sorted_keys || !ws || !row_start || !neighbours || !edges || !edge_faces || !edge_forward || !boundary_vertex || !counts)
        return NPCD_ERR_ARG;
    if (misaligned(sorted_keys, 8) || misaligned(ws, 8) || misaligned(counts, 8) || misaligned(row_start, 4) ||
        misaligned(neighbours, 4) || misaligned(edges, 4) || misaligned(edge_faces, 4) || misaligned(edge_forward, 4))
        return NPCD_ERR_ARG;
    SmWs w;
    sm_ws_layout(ws, F, &w);
    SmEdges o{row_start, neighbours, edges, edge_faces, edge_forward, boundary_vertex, V, D};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    NPCD_HIP_CHECK(hipMemsetAsync(boundary_vertex, 0, (size_t)V, s));
    const int64_t strips = sm_strips(6 * F);
    hipLaunchKernelGGL(sm_emit_kernel, dim3((unsigned)strips), dim3(kSmThreads), 0, s, sorted_keys, 6 * F, w, o);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sm_counts_kernel, dim3(1), dim3(kSmThreads), 0, s, w.strip_counts, strips, counts + kSmCountUsed);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int64_t npcd_smooth_ws_bytes(int64_t V) {
    const int rc = sm_check(V, 0);
    if (rc != NPCD_OK) return rc;
    return sm_state_bytes(V);
}

extern "C" int npcd_smooth_mesh(const float* vertices, int64_t V, const int32_t* row_start, const int32_t* neighbours, int64_t D,
                                const uint8_t* boundary_vertex, const uint8_t* fixed, int iterations, double lam, double mu, void* ws,
                                float* vertices_out, void* stream) {
    const int rc = sm_check(V, 0);
    if (rc != NPCD_OK) return rc;
    if (V < 1 || D < 0 || D >= 6 * kSmMaxFaces || iterations < 0 || iterations > kSmMaxIterations) return NPCD_ERR_ARG;
    if (!(lam > 0.0 && lam <= 1.0) || !(mu >= -1.0 && mu <= 0.0)) return NPCD_ERR_ARG;
    if (!vertices || !vertices_out || !row_start || !ws || (D > 0 && !neighbours)) return NPCD_ERR_ARG;
    if (misaligned(vertices, 4) || misaligned(vertices_out, 4) || misaligned(row_start, 4) || misaligned(neighbours, 4) ||
        misaligned(ws, 16))
        return NPCD_ERR_ARG;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (iterations == 0 || D == 0) {          // nothing moves: the input bits
        if (vertices_out != vertices) NPCD_HIP_CHECK(hipMemcpyAsync(vertices_out, vertices, (size_t)V * 12, hipMemcpyDeviceToDevice, s));
        return NPCD_OK;
    }
    SmArgs a{vertices, row_start, neighbours, boundary_vertex, fixed, static_cast<uint32_t*>(ws), vertices_out, V, D};
    SmRecord* state[2] = {reinterpret_cast<SmRecord*>(static_cast<char*>(ws) + 16), nullptr};
    state[1] = state[0] + V;
    const dim3 grid(blocks_for(V, kSmThreads)), block(kSmThreads);
    NPCD_HIP_CHECK(hipMemsetAsync(ws, 0, 16, s));
    hipLaunchKernelGGL(sm_measure_kernel, grid, block, 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sm_quantise_kernel, grid, block, 0, s, a, state[0]);
    NPCD_HIP_CHECK(hipGetLastError());
    int at = 0;
    for (int it = 0; it < iterations; ++it)
        for (int half = 0; half < (mu == 0.0 ? 1 : 2); ++half, at ^= 1) {
            hipLaunchKernelGGL(sm_step_kernel, grid, block, 0, s, a, state[at], state[at ^ 1], half ? mu : lam);
            NPCD_HIP_CHECK(hipGetLastError());
        }
    hipLaunchKernelGGL(sm_finish_kernel, grid, block, 0, s, a, state[at]);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
