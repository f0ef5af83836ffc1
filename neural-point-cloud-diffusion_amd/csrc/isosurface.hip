// Isosurface of a density volume as an indexed triangle mesh: marching tetrahedra on the Kuhn / Freudenthal
// triangulation of the lattice, two passes, no atomics.  The operator under npcd/eval/mesh.py (extract_mesh).
//
//   vol [B, gz, gy, gx] fp32, x fastest; node (x, y, z) has the index (z gy + y) gx + x.  A node is inside iff f > level (NaN: outside).
//   Seven edge types per node by (dx, dy, dz): 0 (1,0,0)  1 (0,1,0)  2 (0,0,1)  3 (1,1,0)  4 (1,0,1)  5 (0,1,1)  6 (1,1,1); the lower
//   end owns the edge.  An edge whose ends differ in "inside" carries one vertex, t = (level - f_lo) / (f_hi - f_lo) along it;
//   vertices in ascending (node, type).  A cell is cut into six tetrahedra, one per permutation (a, b, c) of the axes in
//   lexicographic order: the chain v0, v0 + e_a, v0 + e_a + e_b, v0 + e_a + e_b + e_c.  Every edge of such a chain is one of the
//   seven types, so a triangle's corners are vertices that some node owns.  Triangles in ascending (cell, tetrahedron, triangle).
//
// Winding.  A chain (p0, p1, p2, p3) has det [p1 - p0, p2 - p0, p3 - p0] = the sign of the permutation.  In a positive
// tetrahedron the triangle (e_ij, e_ik, e_il) has its normal pointing away from corner i when (i, j, k, l) is an even permutation
// of (0, 1, 2, 3), and the quadrilateral (e_ik, e_il, e_jl, e_jk) has its normal pointing from {i, j} to {k, l}: iso_case() holds
// these for the 14 mixed corner patterns, inside -> outside.  An odd permutation of the axes reverses them.  Nothing is decided
// from coordinates, so triangles of zero area (a sample equal to `level`) keep their winding.  A triangle is then rotated to start with
// its smallest vertex index; a quadrilateral is rotated likewise and split along the diagonal through that vertex.
//
// Passes.  A workgroup owns a strip of kIsoThreads consecutive node indices, one node per lane -- the output order is the node
// order, so a strip's output is one contiguous range.
//   count: a node reads its own sample and the seven at the upper ends of its edges (the other seven corners of its cell), and
//          writes one word: bits 0-6 the crossed edge types, bit 7 "inside", bits 8.. the vertices of its strip before it
//          (the exclusive form of block_scan, block_scan.h).  The strip's vertex and triangle totals go to two small
//          arrays.
//   scan:  one workgroup per volume turns the strips' totals into exclusive bases, in place, and writes counts[b] = (V, F).
//   emit:  the owner writes its vertices; a cell reads the eight words of its corners -- "inside" bits and vertex bases, the volume is
//          not read again for the faces -- scans the triangle counts over the strip as before and writes its triangles.  The index
//          of a neighbour's vertex is base[strip of the node] + (word >> 8) + popcount(mask & ((1 << type) - 1)).
// What emit writes follows from the words alone: the number of vertices and triangles cannot differ from what count reported,
// whatever `level` or the volume hold at the second call.
//
// Plain loads: consecutive lanes read consecutive nodes; the +gx neighbours are read by the same strip a row later, the +gx gy
// neighbours by the strip one slab later, and come from the caches.  No LDS tile: the output order is the node order, which a strip
// keeps and a three-dimensional tile does not, and the passes are not limited by the loads -- at 256^3 count moves its 8 bytes a
// node at 0.9 TB/s, an eighth of what HBM gives, so the time is in launching and scanning one node per lane (docs/experiments.md
// R30.1, with what would help instead).
//
// Bounds.  A neighbour is read only where the node has one on that axis; a lane past the volume's last node reads and writes
// nothing and scans zeros.  7 gz gy gx < 2^31 (checked), so node, vertex and strip indices are ints; byte offsets and the
// triangle bases are 64 bits.
#include "block_scan.h"
#include "common.h"

namespace npcd {

constexpr int kIsoThreads = 1024;          // nodes per workgroup
constexpr int kIsoWaves = kIsoThreads / kWave;

#define NPCD_ISO_HD __host__ __device__ __forceinline__

// the corner code of an offset is dx | dy << 1 | dz << 2; the edge type of a code, and back
NPCD_ISO_HD constexpr int iso_type_of(int code) { return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 3 ? 3 : code == 5 ? 4 : code == 6 ? 5 : 6; }
NPCD_ISO_HD constexpr int iso_code_of(int type) { return type == 0 ? 1 : type == 1 ? 2 : type == 2 ? 4 : type == 3 ? 3 : type == 4 ? 5 : type == 5 ? 6 : 7; }
// tetrahedron t of a cell is the chain of corner codes 0, c1, c2, 7 for the t-th permutation of (x, y, z)
NPCD_ISO_HD constexpr int iso_c1(int t) { return t < 2 ? 1 : t < 4 ? 2 : 4; }
NPCD_ISO_HD constexpr int iso_c2(int t) { return t == 0 ? 3 : t == 1 ? 5 : t == 2 ? 3 : t == 3 ? 6 : t == 4 ? 5 : 6; }
NPCD_ISO_HD constexpr bool iso_odd(int t) { return t == 1 || t == 2 || t == 5; }          // xzy, yxz, zyx

// in8: bit c = corner c of the cell is inside -> bit i = corner i of the chain is inside
NPCD_ISO_HD int iso_pattern(uint32_t in8, int t) {
    return (int)((in8 & 1) | ((in8 >> iso_c1(t)) & 1) << 1 | ((in8 >> iso_c2(t)) & 1) << 2 | ((in8 >> 7) & 1) << 3);
}
NPCD_ISO_HD int iso_pattern_tris(int pat) {
    const int p = __builtin_popcount((unsigned)pat);
    return p == 2 ? 2 : (p == 1 || p == 3) ? 1 : 0;
}
NPCD_ISO_HD int iso_cell_tris(uint32_t in8) {
    if (in8 == 0 || in8 == 0xff) return 0;
    int n = 0;
    for (int t = 0; t < 6; ++t) n += iso_pattern_tris(iso_pattern(in8, t));
    return n;
}

// The polygon of a corner pattern in a positive chain, as edges of the chain: 0 = 01, 1 = 02, 2 = 03, 3 = 12, 4 = 13, 5 = 23.
// n | e0 << 4 | e1 << 8 | e2 << 12 | e3 << 16, n = 3 or 4 corners, 0 for the two uniform patterns.
NPCD_ISO_HD constexpr uint32_t iso_poly(int n, int e0, int e1, int e2, int e3) {
    return (uint32_t)(n | e0 << 4 | e1 << 8 | e2 << 12 | e3 << 16);
}
NPCD_ISO_HD uint32_t iso_case(int pat) {
    switch (pat) {
        case 1: return iso_poly(3, 0, 1, 2, 0);           // corner 0 inside: (0; 1, 2, 3)
        case 2: return iso_poly(3, 0, 4, 3, 0);           // (1; 0, 3, 2)
        case 4: return iso_poly(3, 1, 3, 5, 0);           // (2; 0, 1, 3)
        case 8: return iso_poly(3, 2, 5, 4, 0);           // (3; 0, 2, 1)
        case 14: return iso_poly(3, 0, 2, 1, 0);          // corner 0 outside: the reverse
        case 13: return iso_poly(3, 0, 3, 4, 0);
        case 11: return iso_poly(3, 1, 5, 3, 0);
        case 7: return iso_poly(3, 2, 4, 5, 0);
        case 3: return iso_poly(4, 1, 2, 4, 3);           // {0, 1} inside: (0, 1, 2, 3) -> 02, 03, 13, 12
        case 5: return iso_poly(4, 2, 0, 3, 5);           // {0, 2}: (0, 2, 3, 1)
        case 9: return iso_poly(4, 0, 1, 5, 4);           // {0, 3}: (0, 3, 1, 2)
        case 6: return iso_poly(4, 0, 4, 5, 1);           // {1, 2}: (1, 2, 0, 3)
        case 10: return iso_poly(4, 3, 0, 2, 5);          // {1, 3}: (1, 3, 2, 0)
        case 12: return iso_poly(4, 1, 3, 4, 2);          // {2, 3}: (2, 3, 0, 1)
        default: return 0;
    }
}
NPCD_ISO_HD int iso_pick(const int* E, int i) {          // E[i] without an indexed register array
    return i == 0 ? E[0] : i == 1 ? E[1] : i == 2 ? E[2] : i == 3 ? E[3] : i == 4 ? E[4] : E[5];
}

// The triangles of one tetrahedron in canonical form: (q0, q1, q2) and, with n = 2, (q0, q2, q3).  E: the vertex index on each of
// the chain's six edges (read only where the pattern crosses the edge).
struct IsoFaces {
    int n, q0, q1, q2, q3;
};
NPCD_ISO_HD IsoFaces iso_tet_faces(int pat, bool odd, const int* E) {
    const uint32_t c = iso_case(pat);
    const int n = (int)(c & 15);
    if (n == 0) return IsoFaces{0, 0, 0, 0, 0};
    const int q0 = iso_pick(E, (c >> 4) & 7), q2 = iso_pick(E, (c >> 12) & 7);
    int q1 = iso_pick(E, (c >> 8) & 7), q3 = n == 4 ? iso_pick(E, (c >> 16) & 7) : q2;
    if (n == 3) {          // an odd permutation of the axes reverses: (q0, q2, q1); the smallest of the three goes first
        const int p1 = odd ? q2 : q1, p2 = odd ? q1 : q2;
        const bool at1 = p1 < q0 && p1 < p2, at2 = p2 < q0 && p2 < p1;
        return IsoFaces{1, at1 ? p1 : at2 ? p2 : q0, at1 ? p2 : at2 ? q0 : p1, at1 ? q0 : at2 ? p1 : p2, 0};
    }
    if (odd) { const int s = q1; q1 = q3; q3 = s; }          // (q0, q3, q2, q1)
    const int a = q0 < q1 ? q0 : q1, b = q2 < q3 ? q2 : q3, lowest = a < b ? a : b;          // the four are distinct
    const bool at0 = q0 == lowest, at1 = q1 == lowest, at2 = q2 == lowest;
    return IsoFaces{2, lowest, at0 ? q1 : at1 ? q2 : at2 ? q3 : q0, at0 ? q2 : at1 ? q3 : at2 ? q0 : q1, at0 ? q3 : at1 ? q0 : at2 ? q1 : q2};
}

struct IsoArgs {
    const float* vol;                  // [B, n]
    uint32_t* words;                   // [B, n]
    int32_t* wg_verts;                 // [B, W] totals, then exclusive bases
    int64_t* wg_tris;                  // [B, W]
    int64_t* counts;                   // [B, 2]
    const int64_t *vert_off, *face_off;          // [B]
    float* vertices;                   // [sum V, 3]
    int32_t* faces;                    // [sum F, 3]
    float level, origin[3], spacing[3];
    int gx, gy, gz, n, W;
};

struct IsoNode {
    int node, x, y, z;
    bool valid, hx, hy, hz;          // in the volume; has a neighbour at +1 on the axis
    int sx, sy;                      // node strides of y and z
    __device__ __forceinline__ bool has(int code) const {
        return valid && (!(code & 1) || hx) && (!(code & 2) || hy) && (!(code & 4) || hz);
    }
    __device__ __forceinline__ int off(int code) const { return (code & 1) + ((code >> 1) & 1) * sx + ((code >> 2) & 1) * sy; }
    __device__ __forceinline__ bool cell() const { return valid && hx && hy && hz; }
};
__device__ __forceinline__ IsoNode iso_node(const IsoArgs& a, int wg, int tid) {
    IsoNode p;
    p.node = wg * kIsoThreads + tid;
    p.valid = p.node < a.n;
    const int row = p.node / a.gx;
    p.x = p.node - row * a.gx;
    p.z = row / a.gy;
    p.y = row - p.z * a.gy;
    p.hx = p.x + 1 < a.gx, p.hy = p.y + 1 < a.gy, p.hz = p.z + 1 < a.gz;
    p.sx = a.gx, p.sy = a.gx * a.gy;
    return p;
}

__global__ __launch_bounds__(kIsoThreads) void iso_count_kernel(IsoArgs a) {
    __shared__ uint64_t wave_total[kIsoWaves];
    const int b = blockIdx.x / a.W, wg = blockIdx.x - b * a.W;
    const IsoNode p = iso_node(a, wg, threadIdx.x);
    uint32_t in8 = 0, mask = 0;
    if (p.valid) {
        const float* v = a.vol + (int64_t)b * a.n + p.node;
        in8 = v[0] > a.level;
#pragma unroll
        for (int c = 1; c < 8; ++c)
            if (p.has(c)) in8 |= (uint32_t)(v[p.off(c)] > a.level) << c;
#pragma unroll
        for (int c = 1; c < 8; ++c)
            if (p.has(c) && ((in8 >> c) & 1) != (in8 & 1)) mask |= 1u << iso_type_of(c);
    }
    const uint32_t nv = __builtin_popcount(mask), nt = p.cell() ? iso_cell_tris(in8) : 0;
    uint64_t total;
    const uint64_t before = block_scan<kIsoThreads, false>((uint64_t)nt << 32 | nv, wave_total, &total);
    if (p.valid) a.words[(int64_t)b * a.n + p.node] = mask | (in8 & 1) << 7 | (uint32_t)before << 8;
    if (threadIdx.x == 0) {
        a.wg_verts[blockIdx.x] = (int32_t)(uint32_t)total;
        a.wg_tris[blockIdx.x] = (int64_t)(total >> 32);
    }
}

__global__ __launch_bounds__(kIsoThreads) void iso_scan_kernel(IsoArgs a) {
    __shared__ uint64_t wave_total[kIsoWaves];
    int32_t* const verts = a.wg_verts + (int64_t)blockIdx.x * a.W;
    int64_t* const tris = a.wg_tris + (int64_t)blockIdx.x * a.W;
    uint64_t carry_v = 0, carry_t = 0;          // workgroup-uniform
    for (int base = 0; base < a.W; base += kIsoThreads) {
        const int i = base + threadIdx.x;
        const bool live = i < a.W;
        const uint64_t v = live ? (uint64_t)verts[i] : 0, t = live ? (uint64_t)tris[i] : 0;
        uint64_t total_v, total_t;
        const uint64_t before_v = block_scan<kIsoThreads, false>(v, wave_total, &total_v);
        const uint64_t before_t = block_scan<kIsoThreads, false>(t, wave_total, &total_t);
        if (live) {
            verts[i] = (int32_t)(carry_v + before_v);
            tris[i] = (int64_t)(carry_t + before_t);
        }
        carry_v += total_v, carry_t += total_t;
    }
    if (threadIdx.x == 0) {
        a.counts[2 * blockIdx.x] = (int64_t)carry_v;
        a.counts[2 * blockIdx.x + 1] = (int64_t)carry_t;
    }
}

// the index of the vertex on the edge between corners LO and HI of a cell (corner codes, LO a subset of HI): w / vb = the words and the
// vertex bases of the cell's eight corners
template <int LO, int HI>
__device__ __forceinline__ int iso_edge_vertex(const uint32_t (&w)[8], const int (&vb)[8]) {
    return vb[LO] + __builtin_popcount(w[LO] & ((1u << iso_type_of(LO ^ HI)) - 1));
}
// tetrahedron T of a cell: its triangles to f; returns where the next one goes
template <int T>
__device__ __forceinline__ int32_t* iso_emit_tet(uint32_t in8, const uint32_t (&w)[8], const int (&vb)[8], int32_t* f) {
    const int pat = iso_pattern(in8, T);
    if (pat == 0 || pat == 15) return f;
    constexpr int c1 = iso_c1(T), c2 = iso_c2(T);
    const int E[6] = {iso_edge_vertex<0, c1>(w, vb), iso_edge_vertex<0, c2>(w, vb), iso_edge_vertex<0, 7>(w, vb),
                      iso_edge_vertex<c1, c2>(w, vb), iso_edge_vertex<c1, 7>(w, vb), iso_edge_vertex<c2, 7>(w, vb)};
    const IsoFaces k = iso_tet_faces(pat, iso_odd(T), E);
    f[0] = k.q0, f[1] = k.q1, f[2] = k.q2;
    if (k.n == 2) f[3] = k.q0, f[4] = k.q2, f[5] = k.q3;
    return f + 3 * k.n;
}

__global__ __launch_bounds__(kIsoThreads) void iso_emit_kernel(IsoArgs a) {
    __shared__ uint64_t wave_total[kIsoWaves];
    const int b = blockIdx.x / a.W, wg = blockIdx.x - b * a.W;
    const IsoNode p = iso_node(a, wg, threadIdx.x);
    const uint32_t* const words = a.words + (int64_t)b * a.n;
    const int32_t* const bases = a.wg_verts + (int64_t)b * a.W;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, in8 = 0;
    int vb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.valid) {
        w[0] = words[p.node];
        vb[0] = bases[wg] + (int)(w[0] >> 8);
        if (w[0] & 0x7f) {
            const float* v = a.vol + (int64_t)b * a.n + p.node;
            const float f_lo = v[0];
            float* out = a.vertices + (a.vert_off[b] + vb[0]) * 3;
#pragma unroll
            for (int type = 0; type < 7; ++type) {
                const int c = iso_code_of(type);
                if ((w[0] >> type) & 1) {
                    const float f_hi = v[p.off(c)];
                    const float t = (a.level - f_lo) / (f_hi - f_lo);
                    const float g0 = (float)p.x + ((c & 1) ? t : 0.f), g1 = (float)p.y + ((c & 2) ? t : 0.f),
                                g2 = (float)p.z + ((c & 4) ? t : 0.f);
                    out[0] = a.origin[0] + a.spacing[0] * g0;
                    out[1] = a.origin[1] + a.spacing[1] * g1;
                    out[2] = a.origin[2] + a.spacing[2] * g2;
                    out += 3;
                }
            }
        }
        if (p.cell()) {
            in8 = (w[0] >> 7) & 1;
#pragma unroll
            for (int c = 1; c < 8; ++c) {
                const int nd = p.node + p.off(c);
                w[c] = words[nd];
                vb[c] = bases[nd / kIsoThreads] + (int)(w[c] >> 8);
                in8 |= ((w[c] >> 7) & 1) << c;
            }
        }
    }
    const int nt = iso_cell_tris(in8);          // 0 off the cells: in8 is 0 there
    uint64_t total;
    const uint64_t before = block_scan<kIsoThreads, false>((uint64_t)nt, wave_total, &total);
    if (nt) {
        int32_t* f = a.faces + (a.face_off[b] + a.wg_tris[blockIdx.x] + (int64_t)before) * 3;
        f = iso_emit_tet<0>(in8, w, vb, f);
        f = iso_emit_tet<1>(in8, w, vb, f);
        f = iso_emit_tet<2>(in8, w, vb, f);
        f = iso_emit_tet<3>(in8, w, vb, f);
        f = iso_emit_tet<4>(in8, w, vb, f);
        iso_emit_tet<5>(in8, w, vb, f);
    }
}

// node count and strips per volume; the sizes the entry points refuse
static inline int iso_check(int B, int gz, int gy, int gx, int* n, int* W) {
    if (B <= 0 || gz < 2 || gy < 2 || gx < 2) return NPCD_ERR_ARG;
    const int64_t slab = (int64_t)gy * gx;
    if (slab >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    const int64_t nodes = slab * gz;
    if (7 * nodes >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    const int64_t strips = (nodes + kIsoThreads - 1) / kIsoThreads;
    if (strips * B >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    *n = (int)nodes, *W = (int)strips;
    return NPCD_OK;
}

// workspace: wg_tris int64 [B, W] | words [B, n] | wg_verts [B, W]
static inline int64_t iso_ws_bytes(int B, int n, int W) { return (int64_t)B * W * 12 + (int64_t)B * n * 4; }
static inline void iso_ws(IsoArgs* a, void* ws, int B) {
    a->wg_tris = static_cast<int64_t*>(ws);
    a->words = reinterpret_cast<uint32_t*>(a->wg_tris + (int64_t)B * a->W);
    a->wg_verts = reinterpret_cast<int32_t*>(a->words + (int64_t)B * a->n);
}

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_isosurface_ws_bytes(int B, int gz, int gy, int gx) {
    int n, W;
    const int rc = iso_check(B, gz, gy, gx, &n, &W);
    return rc != NPCD_OK ? rc : iso_ws_bytes(B, n, W);
}

extern "C" int npcd_isosurface_count(const float* vol, int B, int gz, int gy, int gx, float level, void* ws, int64_t* counts, void* stream) {
    IsoArgs a{};
    const int rc = iso_check(B, gz, gy, gx, &a.n, &a.W);
    if (rc != NPCD_OK) return rc;
    if (!vol || !ws || !counts || (reinterpret_cast<uintptr_t>(ws) & 7)) return NPCD_ERR_ARG;
    a.vol = vol, a.counts = counts, a.level = level, a.gx = gx, a.gy = gy, a.gz = gz;
    iso_ws(&a, ws, B);
    hipLaunchKernelGGL(iso_count_kernel, dim3((unsigned)(B * a.W)), dim3(kIsoThreads), 0, static_cast<hipStream_t>(stream), a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(iso_scan_kernel, dim3((unsigned)B), dim3(kIsoThreads), 0, static_cast<hipStream_t>(stream), a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}

extern "C" int npcd_isosurface_emit(const float* vol, int B, int gz, int gy, int gx, float level, const float* origin_host,
                                    const float* spacing_host, const void* ws, const int64_t* vert_offsets, const int64_t* face_offsets,
                                    float* vertices, int32_t* faces, void* stream) {
    IsoArgs a{};
    const int rc = iso_check(B, gz, gy, gx, &a.n, &a.W);
    if (rc != NPCD_OK) return rc;
    if (!vol || !origin_host || !spacing_host || !ws || !vert_offsets || !face_offsets || !vertices || !faces ||
        (reinterpret_cast<uintptr_t>(ws) & 7))
        return NPCD_ERR_ARG;
    a.vol = vol, a.level = level, a.gx = gx, a.gy = gy, a.gz = gz;
    a.vert_off = vert_offsets, a.face_off = face_offsets, a.vertices = vertices, a.faces = faces;
    for (int i = 0; i < 3; ++i) a.origin[i] = origin_host[i], a.spacing[i] = spacing_host[i];
    iso_ws(&a, const_cast<void*>(ws), B);
    hipLaunchKernelGGL(iso_emit_kernel, dim3((unsigned)(B * a.W)), dim3(kIsoThreads), 0, static_cast<hipStream_t>(stream), a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
