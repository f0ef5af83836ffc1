// Area-weighted sampling of triangle meshes: a batch of meshes packed as concatenated vertices and faces with
// vert_offsets / face_offsets [B + 1] on the device.  The per-lane arithmetic is csrc/surface.h, shared with the host program
// csrc/surface_host.cpp; this file is the launches around it.  Compiled without FMA contraction (build.py).
//
//   npcd_surface_prepare, three launches:
//     measure   one workgroup per tile slot (surf_tile_base: kSurfTile consecutive faces of one mesh), one lane per face: d = |e1 x e2|
//               to the workspace, and the integer maximum of its bits into the mesh's word (wave_publish_max of csrc/wave.h; d >= +0,
//               so the bits order as the values do).
//     quantise  the same grid: w = floor(float64(d) 2^k), the inclusive sums of w inside the tile (block_scan of
//               csrc/block_scan.h) to the workspace, the tile's total to its slot.
//     tiles     one workgroup per mesh: the inclusive sums of its tile totals in place (block_scan_totals); W and the area.
//   npcd_surface_sample, one launch: one lane per sample (surf_sample_row).  The mesh's tile sums are staged in LDS where they fit
//               (kSurfLdsTiles), the second search reads the tile's local sums from global memory.
//   Integer sums throughout: the order of the additions does not matter, and no workgroup waits on another -- the launches are the
//   only ordering.  Every store is an ordinary vector store.
//
// Bounds.  A member's rows are taken through surf_span: offsets that do not ascend inside [0, total] give an empty member.  A lane past
// the mesh's last face, tile or sample reads and writes nothing (its weight in a scan is 0).  A face index outside [0, V) is not
// followed (surf_face).  Tile slots: blockIdx.x < floor(F_total / kSurfTile) + B, the size of the slot arrays.
#include "block_scan.h"
#include "common.h"
#include "surface.h"

namespace npcd {

struct SurfWs {          // the workspace: 8-byte aligned base
    uint64_t *local, *tiles, *mesh_W;          // [F_total], [slots], [B]
    float* d;                                   // [F_total]
    uint32_t* d_max;                            // [B]
};
static inline int64_t surf_ws_layout(void* ws, int B, int F_total, SurfWs* out) {
    const int64_t slots = surf_slots(B, F_total);
    unsigned char* p = static_cast<unsigned char*>(ws);
    out->local = reinterpret_cast<uint64_t*>(p);
    out->tiles = out->local + F_total;
    out->mesh_W = out->tiles + slots;
    out->d = reinterpret_cast<float*>(out->mesh_W + B);
    out->d_max = reinterpret_cast<uint32_t*>(out->d + F_total);
    return 8 * ((int64_t)F_total + slots + B) + 4 * ((int64_t)F_total + B);
}

struct SurfArgs {
    const float* vertices;
    const int32_t *faces, *vert_off, *face_off;
    SurfWs ws;
    double* area;
    int B, V_total, F_total;
    // the sample launch
    const float *u, *vnormals, *attrs;
    float *points, *normals_out, *attrs_out;
    int32_t* faces_out;
    int S, C, normals_mode;
};

// the mesh and the tile of this workgroup's slot; false for a slot no mesh uses
__device__ __forceinline__ bool surf_slot(const SurfArgs& a, int* b, SurfSpan* fs, int* tile) {
    *b = surf_slot_member(a.face_off, a.B, blockIdx.x);
    *fs = surf_span(a.face_off, *b, a.F_total);
    const int64_t t = (int64_t)blockIdx.x - surf_tile_base(a.face_off[*b], *b);
    *tile = (int)t;
    return t >= 0 && t < surf_tiles(fs->count);
}

__global__ __launch_bounds__(kSurfThreads) void surf_measure_kernel(SurfArgs a) {
    int b, tile;
    SurfSpan fs;
    if (!surf_slot(a, &b, &fs, &tile)) return;
    const SurfSpan vs = surf_span(a.vert_off, b, a.V_total);
    const int64_t i = (int64_t)tile * kSurfTile + threadIdx.x;
    uint32_t bits = 0;
    if (i < fs.count) bits = surf_measure_lane(a.vertices + (int64_t)vs.first * 3, a.faces + (int64_t)fs.first * 3, vs.count, (int)i, a.ws.d + fs.first);
    wave_publish_max(bits, a.ws.d_max + b);          // every lane of the wave is here
}

__global__ __launch_bounds__(kSurfThreads) void surf_quantise_kernel(SurfArgs a) {
    __shared__ uint64_t wave_total[kSurfThreads / 64];
    int b, tile;
    SurfSpan fs;
    if (!surf_slot(a, &b, &fs, &tile)) return;
    const int64_t i = (int64_t)tile * kSurfTile + threadIdx.x;
    const uint32_t d_max = a.ws.d_max[b];
    const uint64_t w = i < fs.count ? surf_quantise(a.ws.d[fs.first + i], d_max) : 0;
    uint64_t total;
    const uint64_t incl = block_scan<kSurfThreads, true>(w, wave_total, &total);
    if (i < fs.count) a.ws.local[fs.first + i] = incl;
    if (threadIdx.x == 0) a.ws.tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSurfThreads) void surf_tiles_kernel(SurfArgs a) {
    __shared__ uint64_t wave_total[kSurfThreads / 64];
    const int b = blockIdx.x;
    const SurfSpan fs = surf_span(a.face_off, b, a.F_total);
    const int n = surf_tiles(fs.count);
    uint64_t* tiles = a.ws.tiles + surf_tile_base(fs.first, b);          // (n = 0 for a span that is not one: not followed)
    const uint64_t W = block_scan_totals<kSurfThreads, true>(tiles, n, wave_total);
    if (threadIdx.x == 0) {
        a.ws.mesh_W[b] = W;
        a.area[b] = surf_area(W, a.ws.d_max[b]);
    }
}

__global__ __launch_bounds__(kSurfThreads) void surf_sample_kernel(SurfArgs a) {
    __shared__ uint64_t staged[kSurfLdsTiles];
    const int b = blockIdx.y;
    const SurfSpan fs = surf_span(a.face_off, b, a.F_total), vs = surf_span(a.vert_off, b, a.V_total);
    SurfMesh m;
    m.vertices = a.vertices + (int64_t)vs.first * 3, m.faces = a.faces + (int64_t)fs.first * 3;
    m.local = a.ws.local + fs.first, m.tiles = a.ws.tiles + surf_tile_base(fs.first, b);
    m.vnormals = a.vnormals ? a.vnormals + (int64_t)vs.first * 3 : nullptr;
    m.attrs = a.attrs ? a.attrs + (int64_t)vs.first * a.C : nullptr;
    m.V = vs.count, m.F = fs.count, m.C = a.C, m.normals_mode = a.normals_mode;
    m.W = a.ws.mesh_W[b];
    const int n = surf_tiles(m.F);
    if (m.W && n <= kSurfLdsTiles) {          // the same for every lane of the workgroup
        for (int t = threadIdx.x; t < n; t += kSurfThreads) staged[t] = m.tiles[t];
        __syncthreads();
        m.tiles = staged;
    }
    const int s = blockIdx.x * kSurfThreads + threadIdx.x;
    if (s >= a.S) return;
    const int64_t row = (int64_t)b * a.S + s;
    SurfRow o;
    o.point = a.points + row * 3;
    o.face = a.faces_out ? a.faces_out + row : nullptr;
    o.normal = a.normals_out ? a.normals_out + row * 3 : nullptr;
    o.attr = a.attrs_out ? a.attrs_out + row * a.C : nullptr;
    surf_sample_row(m, a.u + row * 3, o);
}

static int surf_check(int B, int64_t V_total, int64_t F_total) {
    if (B < 1 || V_total < 0 || F_total < 0) return NPCD_ERR_ARG;
    // rows and tile slots are counted with int (elements with int64_t), and a mesh's weights sum below 2^63 only for F < 2^31
    if (V_total >= (int64_t)1 << 31 || F_total >= (int64_t)1 << 31 || F_total / kSurfTile + B >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    return NPCD_OK;
}

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_surface_ws_bytes(int B, int64_t F_total) {
    const int rc = surf_check(B, 0, F_total);
    if (rc != NPCD_OK) return rc;
    SurfWs w;
    return surf_ws_layout(nullptr, B, (int)F_total, &w);
}

extern "C" int npcd_surface_prepare(const float* vertices, const int32_t* faces, const int32_t* vert_offsets, const int32_t* face_offsets, int B,
                                    int64_t V_total, int64_t F_total, void* ws, double* area, void* stream) {
    const int rc = surf_check(B, V_total, F_total);
    if (rc != NPCD_OK) return rc;
    if (!vertices || !faces || !vert_offsets || !face_offsets || !ws || !area) return NPCD_ERR_ARG;
    if (misaligned(ws, 8) || misaligned(area, 8) || misaligned(vertices, 4) || misaligned(faces, 4) || misaligned(vert_offsets, 4) ||
        misaligned(face_offsets, 4))
        return NPCD_ERR_ARG;
    SurfArgs a{};
    a.vertices = vertices, a.faces = faces, a.vert_off = vert_offsets, a.face_off = face_offsets, a.area = area;
    a.B = B, a.V_total = (int)V_total, a.F_total = (int)F_total;
    surf_ws_layout(ws, B, a.F_total, &a.ws);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned slots = (unsigned)surf_slots(B, a.F_total);
    NPCD_HIP_CHECK(hipMemsetAsync(a.ws.d_max, 0, (size_t)B * 4, s));
    hipLaunchKernelGGL(surf_measure_kernel, dim3(slots), dim3(kSurfThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(surf_quantise_kernel, dim3(slots), dim3(kSurfThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(surf_tiles_kernel, dim3((unsigned)B), dim3(kSurfThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_surface_sample(const float* vertices, const int32_t* faces, const int32_t* vert_offsets, const int32_t* face_offsets, int B,
                                   int64_t V_total, int64_t F_total, const void* ws, const float* u, int S, float* points, int32_t* faces_out,
                                   int normals_mode, const float* vertex_normals, float* normals_out, const float* attributes, int C,
                                   float* attributes_out, void* stream) {
    const int rc = surf_check(B, V_total, F_total);
    if (rc != NPCD_OK) return rc;
    if (S < 1 || C < 0 || normals_mode < kSurfNormalsNone || normals_mode > kSurfNormalsVertex) return NPCD_ERR_ARG;
    if (C > kSurfMaxChannels) return NPCD_ERR_UNSUPPORTED;
    if ((int64_t)B * S * (C > 3 ? C : 3) >= (int64_t)1 << 31 || (int64_t)(S + kSurfThreads - 1) / kSurfThreads > 0x7fffffff || B > 65535)
        return NPCD_ERR_UNSUPPORTED;
    if (!vertices || !faces || !vert_offsets || !face_offsets || !ws || !u || !points) return NPCD_ERR_ARG;
    if ((normals_mode != kSurfNormalsNone) != (normals_out != nullptr) || (normals_mode == kSurfNormalsVertex) != (vertex_normals != nullptr))
        return NPCD_ERR_ARG;
    if ((C > 0) != (attributes != nullptr) || (C > 0) != (attributes_out != nullptr)) return NPCD_ERR_ARG;
    if (misaligned(ws, 8)) return NPCD_ERR_ARG;
    SurfArgs a{};
    a.vertices = vertices, a.faces = faces, a.vert_off = vert_offsets, a.face_off = face_offsets;
    a.B = B, a.V_total = (int)V_total, a.F_total = (int)F_total;
    surf_ws_layout(const_cast<void*>(ws), B, a.F_total, &a.ws);
    a.u = u, a.S = S, a.points = points, a.faces_out = faces_out, a.normals_mode = normals_mode, a.vnormals = vertex_normals;
    a.normals_out = normals_out, a.attrs = attributes, a.C = C, a.attrs_out = attributes_out;
    hipLaunchKernelGGL(surf_sample_kernel, dim3(blocks_for(S, kSurfThreads), (unsigned)B), dim3(kSurfThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
