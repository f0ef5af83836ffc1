// Vertex clustering of one triangle mesh on a regular grid.  The per-lane arithmetic is csrc/simplify.h, shared with
// the host program csrc/simplify_host.cpp; this file is the launches around it.  Compiled without FMA contraction (build.py).
//
//   npcd_simplify_cluster, one memset and four launches:
//     mark        one lane per vertex: the key of its cell into vertex_cluster (-1: lost), the place inside the cell to the workspace,
//                 the cell's bit into the occupancy bitmap by an integer OR, and the integer maximum of the bits of the finite |a| of its
//                 attributes (wave_publish_max of csrc/wave.h).
//     rank        one lane per bitmap word: the exclusive sums of the popcounts inside a strip of kSimpStrip words (block_scan of
//                 csrc/block_scan.h), the strip's total to its slot;
//     totals      one workgroup: the exclusive sums of the strip totals in place (block_scan_totals); V' to counts[0].
//     accumulate  one lane per vertex: its cluster = strip + word + the set bits below its own, into vertex_cluster; r, the quantised
//                 attributes and 1 into the cluster's integer sums by 64-bit and 32-bit integer atomics at agent scope.
//   npcd_simplify_faces, one launch: one lane per face, the mapped triple to the workspace and the sort keys of its sorted triple.
//   npcd_simplify_unique, one memset and three launches over the caller's stable order of those keys: one lane per position marks the
//                 face that is the first of its run; the inclusive sums of the marks inside strips of kSimpStrip faces; totals as above,
//                 F' to counts[1].
//   npcd_simplify_emit, two launches: finish, one lane per cluster, the float64 expressions of the representative and the attribute
//                 means; compact, one lane per face, the kept faces and their input indices in input order.
//   Integer ORs, maxima and sums throughout: no result depends on the order of an atomic or a scan, and no workgroup waits on
//   another -- the launches are the only ordering.  Every store is an ordinary vector store.
//
// Bounds.  A lane past the last vertex, word, cluster or face reads and writes nothing (it scans 0).  A key lies in [0, cells) by the
// clamp; a cluster id is below U = min(V, cells), the rows of the sums -- an id that is not (cannot be: a workspace that is not this
// mesh's) is dropped.  A face index outside [0, V) and an entry of `order` outside [0, F) are not followed; a kept face is written
// only below F', the rows of the outputs.
#include "block_scan.h"
#include "common.h"
#include "simplify.h"

namespace npcd {

struct SimpWs {          // the workspace: 8-byte aligned base
    uint64_t* sums;                                            // [U, 3 + C]: S and the attribute sums (two's complement)
    uint32_t *n, *a_max, *bitmap;                              // [U], [1], [words]        -- up to here zeroed by npcd_simplify_cluster
    uint32_t *word_before, *strip_before;                      // [words], [strips(words)]
    int32_t* cluster_key;                                      // [U]
    uint32_t* r;                                               // [V, 3]
    int32_t* mapped;                                           // [F, 3]
    uint32_t *fword, *fstrip;                                  // [F]: inclusive marks of the strip << 1 | mark; [strips(F)]
    int64_t zeroed;                                            // bytes from the base that the cluster call zeroes
};
static inline int64_t simp_rows(int64_t V, int64_t cells) { return V < cells ? V : cells; }
static inline int64_t simp_ws_layout(void* ws, int64_t V, int64_t F, int C, int64_t cells, SimpWs* out) {
    const int64_t U = simp_rows(V, cells), words = simp_words(cells);
    out->sums = static_cast<uint64_t*>(ws);
    out->n = reinterpret_cast<uint32_t*>(out->sums + U * (3 + C));
    out->a_max = out->n + U;
    out->bitmap = out->a_max + 1;
    out->word_before = out->bitmap + words;
    out->strip_before = out->word_before + words;
    out->cluster_key = reinterpret_cast<int32_t*>(out->strip_before + simp_strips(words));
    out->r = reinterpret_cast<uint32_t*>(out->cluster_key + U);
    out->mapped = reinterpret_cast<int32_t*>(out->r + V * 3);
    out->fword = reinterpret_cast<uint32_t*>(out->mapped + F * 3);
    out->fstrip = out->fword + F;
    out->zeroed = 8 * U * (3 + C) + 4 * (U + 1 + words);
    return out->zeroed + 4 * (words + simp_strips(words) + U + 3 * V + 3 * F + F + simp_strips(F));
}

struct SimpArgs {
    const float *vertices, *attrs;
    const int32_t* faces;
    SimpGrid g;
    SimpWs ws;
    int32_t* vertex_cluster;
    int64_t *key_hi, *key_lo;
    const int64_t* order;
    float *vertices_out, *attrs_out;
    int32_t *faces_out, *face_source;
    int V, F, C, U, Vp, Fp;
    int64_t words;
};

__global__ __launch_bounds__(kSimpThreads) void simp_mark_kernel(SimpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
    uint32_t bits = 0;
    if (i < a.V) {
        uint32_t r[3];
        const int32_t key = simp_mark_lane(a.vertices + i * 3, a.g, r);
        a.vertex_cluster[i] = key;
        a.ws.r[i * 3] = r[0], a.ws.r[i * 3 + 1] = r[1], a.ws.r[i * 3 + 2] = r[2];
        if (key >= 0) __hip_atomic_fetch_or(a.ws.bitmap + (key >> 5), 1u << (key & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int c = 0; c < a.C; ++c) {
            const uint32_t m = finite_abs_bits(a.attrs[i * a.C + c]);
            bits = m > bits ? m : bits;
        }
    }
    wave_publish_max(bits, a.ws.a_max);          // every lane of the wave is here
}

__global__ __launch_bounds__(kSimpThreads) void simp_rank_kernel(SimpArgs a) {
    __shared__ uint64_t wave_total[kSimpThreads / 64];
    const int64_t w = (int64_t)blockIdx.x * kSimpStrip + threadIdx.x;
    const uint32_t own = w < a.words ? (uint32_t)popcount32(a.ws.bitmap[w]) : 0u;
    uint64_t total;
    const uint32_t before = (uint32_t)block_scan<kSimpThreads, false>(own, wave_total, &total);
    if (w < a.words) a.ws.word_before[w] = before;
    if (threadIdx.x == 0) a.ws.strip_before[blockIdx.x] = (uint32_t)total;
}

// one workgroup: totals [n] to their exclusive sums in place, the sum of all to *out
__global__ __launch_bounds__(kSimpThreads) void simp_totals_kernel(uint32_t* totals, int64_t n, int64_t* out) {
    __shared__ uint64_t wave_total[kSimpThreads / 64];
    const uint64_t sum = block_scan_totals<kSimpThreads, false>(totals, n, wave_total);
    if (threadIdx.x == 0) *out = (int64_t)sum;
}

__global__ __launch_bounds__(kSimpThreads) void simp_accumulate_kernel(SimpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (i >= a.V) return;
    const int32_t key = a.vertex_cluster[i];
    if (key < 0) return;          // lost: stays -1
    const int32_t id = simp_cluster_of(key, a.ws.bitmap, a.ws.word_before, a.ws.strip_before);
    if (id < 0 || id >= a.U) {          // (cannot be)
        a.vertex_cluster[i] = -1;
        return;
    }
    a.vertex_cluster[i] = id;
    a.ws.cluster_key[id] = key;          // every vertex of the cluster stores the same word
    uint64_t* row = a.ws.sums + (int64_t)id * (3 + a.C);
    for (int k = 0; k < 3; ++k) __hip_atomic_fetch_add(row + k, (uint64_t)a.ws.r[i * 3 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a.ws.n + id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t a_max = *a.ws.a_max;
    for (int c = 0; c < a.C; ++c) {
        const int64_t q = simp_quantise(a.attrs[i * a.C + c], a_max);
        if (q) __hip_atomic_fetch_add(row + 3 + c, (uint64_t)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kSimpThreads) void simp_faces_kernel(SimpArgs a) {
    const int64_t f = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (f >= a.F) return;
    int32_t m[3];
    simp_face_lane(a.faces + f * 3, a.vertex_cluster, a.V, m);
    a.ws.mapped[f * 3] = m[0], a.ws.mapped[f * 3 + 1] = m[1], a.ws.mapped[f * 3 + 2] = m[2];
    simp_face_keys(m, a.key_hi ? a.key_hi + f : nullptr, a.key_lo + f);
}

__global__ __launch_bounds__(kSimpThreads) void simp_unique_kernel(SimpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (i >= a.F) return;
    int64_t face;
    if (simp_keeps(a.order, i, a.ws.mapped, a.F, &face)) a.ws.fword[face] = 1u;          // the others keep the memset's 0
}

__global__ __launch_bounds__(kSimpThreads) void simp_flags_kernel(SimpArgs a) {
    __shared__ uint64_t wave_total[kSimpThreads / 64];
    const int64_t f = (int64_t)blockIdx.x * kSimpStrip + threadIdx.x;
    const uint32_t own = f < a.F ? a.ws.fword[f] & 1u : 0u;
    uint64_t total;
    const uint32_t incl = (uint32_t)block_scan<kSimpThreads, true>(own, wave_total, &total);
    if (f < a.F) a.ws.fword[f] = incl << 1 | own;
    if (threadIdx.x == 0) a.ws.fstrip[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(kSimpThreads) void simp_finish_kernel(SimpArgs a) {
    const int64_t id = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (id >= a.Vp) return;
    const uint64_t* row = a.ws.sums + id * (3 + a.C);
    const uint32_t n = a.ws.n[id];
    simp_position(a.ws.cluster_key[id], row, n, a.g, a.vertices_out + id * 3);
    const uint32_t a_max = *a.ws.a_max;
    for (int c = 0; c < a.C; ++c) a.attrs_out[id * a.C + c] = simp_attr_mean((int64_t)row[3 + c], n, a_max);
}

__global__ __launch_bounds__(kSimpThreads) void simp_compact_kernel(SimpArgs a) {
    const int64_t f = (int64_t)blockIdx.x * kSimpThreads + threadIdx.x;
    if (f >= a.F) return;
    const uint32_t w = a.ws.fword[f];
    if (!(w & 1u)) return;
    const int64_t to = (int64_t)a.ws.fstrip[f / kSimpStrip] + (w >> 1) - 1;
    if (to < 0 || to >= a.Fp) return;          // (cannot be)
    for (int k = 0; k < 3; ++k) a.faces_out[to * 3 + k] = a.ws.mapped[f * 3 + k];
    a.face_source[to] = (int32_t)f;
}

static int simp_check(int64_t V, int64_t F, int C, const double* origin, const double* cell, const int* dims, int64_t* cells) {
    if (V < 0 || F < 0 || C < 0 || !dims) return NPCD_ERR_ARG;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return NPCD_ERR_ARG;
    for (int a = 0; a < 3; ++a) {
        if (cell && !(cell[a] > 0.0 && cell[a] < INFINITY)) return NPCD_ERR_ARG;
        if (origin && !(fabs(origin[a]) < INFINITY)) return NPCD_ERR_ARG;
    }
    if (C > kSimpMaxChannels) return NPCD_ERR_UNSUPPORTED;
    // rows are counted with int (elements with int64_t); the cluster sums stay below 2^63 only for V < 2^31
    if (V >= (int64_t)1 << 31 || F >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    if ((int64_t)dims[0] * dims[1] > kSimpMaxCells || (int64_t)dims[0] * dims[1] * dims[2] > kSimpMaxCells) return NPCD_ERR_UNSUPPORTED;
    *cells = simp_cells(dims);
    return NPCD_OK;
}
static void simp_grid(SimpArgs* a, const double* origin, const double* cell, const int* dims) {
    for (int k = 0; k < 3; ++k) a->g.origin[k] = origin[k], a->g.cell[k] = cell[k], a->g.dims[k] = dims[k];
}

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_simplify_ws_bytes(int64_t V, int64_t F, int C, const int* dims_host) {
    int64_t cells;
    const int rc = simp_check(V, F, C, nullptr, nullptr, dims_host, &cells);
    if (rc != NPCD_OK) return rc;
    SimpWs w;
    return simp_ws_layout(nullptr, V, F, C, cells, &w);
}

extern "C" int npcd_simplify_cluster(const float* vertices, int64_t V, int64_t F, const float* attributes, int C, const double* origin_host,
                                     const double* cell_host, const int* dims_host, void* ws, int32_t* vertex_cluster, int64_t* counts,
                                     void* stream) {
    if (!origin_host || !cell_host) return NPCD_ERR_ARG;
    int64_t cells;
    const int rc = simp_check(V, F, C, origin_host, cell_host, dims_host, &cells);
    if (rc != NPCD_OK) return rc;
    if (V < 1 || !vertices || !ws || !vertex_cluster || !counts || (C > 0) != (attributes != nullptr)) return NPCD_ERR_ARG;
    if (misaligned(ws, 8) || misaligned(counts, 8) || misaligned(vertices, 4) || misaligned(vertex_cluster, 4) ||
        misaligned(attributes, 4))
        return NPCD_ERR_ARG;
    SimpArgs a{};
    a.vertices = vertices, a.attrs = attributes, a.vertex_cluster = vertex_cluster;
    a.V = (int)V, a.F = (int)F, a.C = C, a.U = (int)simp_rows(V, cells), a.words = simp_words(cells);
    simp_grid(&a, origin_host, cell_host, dims_host);
    simp_ws_layout(ws, V, F, C, cells, &a.ws);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t strips = simp_strips(a.words);
    NPCD_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)a.ws.zeroed, s));
    hipLaunchKernelGGL(simp_mark_kernel, dim3(blocks_for(V, kSimpThreads)), dim3(kSimpThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(simp_rank_kernel, dim3((unsigned)strips), dim3(kSimpThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(simp_totals_kernel, dim3(1), dim3(kSimpThreads), 0, s, a.ws.strip_before, strips, counts);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(simp_accumulate_kernel, dim3(blocks_for(V, kSimpThreads)), dim3(kSimpThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_simplify_faces(const int32_t* faces, int64_t V, int64_t F, int C, const int* dims_host, const int32_t* vertex_cluster,
                                   void* ws, int64_t* key_hi, int64_t* key_lo, void* stream) {
    int64_t cells;
    const int rc = simp_check(V, F, C, nullptr, nullptr, dims_host, &cells);
    if (rc != NPCD_OK) return rc;
    if (V < 1 || F < 1 || !faces || !vertex_cluster || !ws || !key_lo) return NPCD_ERR_ARG;
    if (misaligned(ws, 8) || misaligned(key_hi, 8) || misaligned(key_lo, 8) || misaligned(faces, 4) ||
        misaligned(vertex_cluster, 4))
        return NPCD_ERR_ARG;
    // one packed key holds cluster ids below 2^21 only: with more rows than that the caller sorts by two keys
    if (!key_hi && simp_rows(V, cells) > kSimpPackedIds) return NPCD_ERR_ARG;
    SimpArgs a{};
    a.faces = faces, a.vertex_cluster = const_cast<int32_t*>(vertex_cluster), a.key_hi = key_hi, a.key_lo = key_lo;
    a.V = (int)V, a.F = (int)F, a.C = C;
    simp_ws_layout(ws, V, F, C, cells, &a.ws);
    hipLaunchKernelGGL(simp_faces_kernel, dim3(blocks_for(F, kSimpThreads)), dim3(kSimpThreads), 0, static_cast<hipStream_t>(stream),
                       a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_simplify_unique(const int64_t* order, int64_t V, int64_t F, int C, const int* dims_host, void* ws, int64_t* counts,
                                    void* stream) {
    int64_t cells;
    const int rc = simp_check(V, F, C, nullptr, nullptr, dims_host, &cells);
    if (rc != NPCD_OK) return rc;
    if (V < 1 || F < 1 || !order || !ws || !counts) return NPCD_ERR_ARG;
    if (misaligned(ws, 8) || misaligned(order, 8) || misaligned(counts, 8)) return NPCD_ERR_ARG;
    SimpArgs a{};
    a.order = order, a.V = (int)V, a.F = (int)F, a.C = C;
    simp_ws_layout(ws, V, F, C, cells, &a.ws);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t strips = simp_strips(F);
    NPCD_HIP_CHECK(hipMemsetAsync(a.ws.fword, 0, (size_t)F * 4, s));
    hipLaunchKernelGGL(simp_unique_kernel, dim3(blocks_for(F, kSimpThreads)), dim3(kSimpThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(simp_flags_kernel, dim3((unsigned)strips), dim3(kSimpThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(simp_totals_kernel, dim3(1), dim3(kSimpThreads), 0, s, a.ws.fstrip, strips, counts + 1);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_simplify_emit(int64_t V, int64_t F, int C, const double* origin_host, const double* cell_host, const int* dims_host,
                                  const void* ws, int64_t V_out, int64_t F_out, float* vertices_out, float* attributes_out,
                                  int32_t* faces_out, int32_t* face_source, void* stream) {
    if (!origin_host || !cell_host) return NPCD_ERR_ARG;
    int64_t cells;
    const int rc = simp_check(V, F, C, origin_host, cell_host, dims_host, &cells);
    if (rc != NPCD_OK) return rc;
    if (V < 1 || !ws || misaligned(ws, 8)) return NPCD_ERR_ARG;
    if (V_out < 1 || V_out > simp_rows(V, cells) || F_out < 0 || F_out > F) return NPCD_ERR_ARG;
    if (!vertices_out || (C > 0) != (attributes_out != nullptr) || (F_out > 0) != (faces_out != nullptr) ||
        (F_out > 0) != (face_source != nullptr))
        return NPCD_ERR_ARG;
    if (misaligned(vertices_out, 4) || misaligned(attributes_out, 4) || misaligned(faces_out, 4) ||
        misaligned(face_source, 4))
        return NPCD_ERR_ARG;
    SimpArgs a{};
    a.V = (int)V, a.F = (int)F, a.C = C, a.U = (int)simp_rows(V, cells), a.Vp = (int)V_out, a.Fp = (int)F_out;
    a.vertices_out = vertices_out, a.attrs_out = attributes_out, a.faces_out = faces_out, a.face_source = face_source;
    simp_grid(&a, origin_host, cell_host, dims_host);
    simp_ws_layout(const_cast<void*>(ws), V, F, C, cells, &a.ws);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(simp_finish_kernel, dim3(blocks_for(V_out, kSimpThreads)), dim3(kSimpThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    if (F_out > 0) {
        hipLaunchKernelGGL(simp_compact_kernel, dim3(blocks_for(F, kSimpThreads)), dim3(kSimpThreads), 0, s, a);
        NPCD_HIP_CHECK(hipGetLastError());
    }
    return NPCD_OK;
}
