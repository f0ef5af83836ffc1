// Vertex normals of the isosurface: the gradient of a field, interpolated along the edge that owns the vertex.  One
// launch beside npcd_isosurface_emit (csrc/isosurface.hip), in a file of its own so that the count / scan / emit kernels and their
// code stay as they are.
//
//   It reads the workspace npcd_isosurface_count left and enumerates the vertices as emit does: a workgroup owns a strip of
//   kIsoStrip consecutive node indices, one node per lane; the node's word holds its crossed edge types (bits 0-6) and the vertices
//   of its strip before it (bits 8..), wg_verts the strip's exclusive vertex base; a node's vertices ascend in the edge type.
//   Node gradient of `field`, per axis, fp32 as written: (f[i + 1] - f[i - 1]) / (2 s) in the interior, (f[1] - f[0]) / (1 s) and
//   (f[last] - f[last - 1]) / (1 s) at the borders.  The vertex on the edge (lo, hi): t = (level - f_lo) / (f_hi - f_lo) from `vol`,
//   as emit computes it; g = g_lo + t (g_hi - g_lo); n2 = (gx gx + gy gy) + gz gz; n = (-g) / sqrt(n2), the division and the root
//   correctly rounded; a vertex with a component that is not finite gets (+0, +0, +0).  Compiled without contraction (build.py).
//
// Bounds.  A lane past the volume's last node reads and writes nothing.  An edge is crossed only where the node has the neighbour,
// so the upper end is a node of the volume; a gradient reads i - 1 and i + 1 only where they exist.  The rows written are those of
// emit: vert_offsets[b] + the strip's base + the node's count before it + the rank of the type among the crossed ones.
#include "common.h"

namespace npcd {

constexpr int kIsoStrip = 1024;          // kIsoThreads of csrc/isosurface.hip (tests/test_components_cpu.py holds the two equal)

struct IsoNormalArgs {
    const float *vol, *field;          // [B, n]
    const uint32_t* words;             // [B, n]
    const int32_t* wg_verts;           // [B, W] exclusive bases
    const int64_t* vert_off;           // [B]
    float* normals;                    // [sum V, 3]
    float level, spacing[3];
    int gx, gy, gz, n, W;
};

// d field / d axis at coordinate i of an axis with `count` nodes and stride `stride`; p points at the node
__device__ __forceinline__ float iso_axis_gradient(const float* p, int i, int count, int stride, float s) {
    if (i == 0) return (p[stride] - p[0]) / (1.f * s);
    if (i == count - 1) return (p[0] - p[-stride]) / (1.f * s);
    return (p[stride] - p[-stride]) / (2.f * s);
}

__global__ __launch_bounds__(kIsoStrip) void iso_normals_kernel(IsoNormalArgs a) {
    const int b = blockIdx.x / a.W, wg = blockIdx.x - b * a.W;
    const int node = wg * kIsoStrip + threadIdx.x;
    if (node >= a.n) return;
    const uint32_t w = a.words[(int64_t)b * a.n + node];
    if (!(w & 0x7f)) return;
    const int row = node / a.gx, x = node - row * a.gx, z = row / a.gy, y = row - z * a.gy;
    const int sy = a.gx, sz = a.gx * a.gy;
    const float* v = a.vol + (int64_t)b * a.n + node;
    const float* f = a.field + (int64_t)b * a.n + node;
    const float f_lo = v[0];
    const float lo0 = iso_axis_gradient(f, x, a.gx, 1, a.spacing[0]), lo1 = iso_axis_gradient(f, y, a.gy, sy, a.spacing[1]),
                lo2 = iso_axis_gradient(f, z, a.gz, sz, a.spacing[2]);
    float* out = a.normals + (a.vert_off[b] + a.wg_verts[(int64_t)b * a.W + wg] + (int64_t)(w >> 8)) * 3;
#pragma unroll
    for (int type = 0; type < 7; ++type) {
        // the corner code dx | dy << 1 | dz << 2 of the type's upper end: 1 2 4 3 5 6 7
        const int c = type == 0 ? 1 : type == 1 ? 2 : type == 2 ? 4 : type == 3 ? 3 : type == 4 ? 5 : type == 5 ? 6 : 7;
        if (!((w >> type) & 1)) continue;
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2, off = dx + dy * sy + dz * sz;
        const float t = (a.level - f_lo) / (v[off] - f_lo);
        const float hi0 = iso_axis_gradient(f + off, x + dx, a.gx, 1, a.spacing[0]), hi1 = iso_axis_gradient(f + off, y + dy, a.gy, sy, a.spacing[1]),
                    hi2 = iso_axis_gradient(f + off, z + dz, a.gz, sz, a.spacing[2]);
        const float g0 = lo0 + t * (hi0 - lo0), g1 = lo1 + t * (hi1 - lo1), g2 = lo2 + t * (hi2 - lo2);
        // sqrtf: v_sqrt_f32 and the two corrections that make it the correctly rounded root (__fsqrt_rn is the bare instruction, 1 ulp)
        const float len = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
        float n0 = -g0 / len, n1 = -g1 / len, n2 = -g2 / len;
        if (!(isfinite(n0) && isfinite(n1) && isfinite(n2))) n0 = n1 = n2 = 0.f;
        out[0] = n0, out[1] = n1, out[2] = n2;
        out += 3;
    }
}

}  // namespace npcd

using namespace npcd;

extern "C" int npcd_isosurface_normals(const float* vol, const float* field, int B, int gz, int gy, int gx, float level,
                                       const float* spacing_host, const void* ws, const int64_t* vert_offsets, float* normals, void* stream) {
    // the sizes npcd_isosurface_count accepts, and its workspace: wg_tris int64 [B, W] | words [B, n] | wg_verts [B, W]
    if (B <= 0 || gz < 2 || gy < 2 || gx < 2) return NPCD_ERR_ARG;
    const int64_t nodes = (int64_t)gz * gy * gx, strips = (nodes + kIsoStrip - 1) / kIsoStrip;
    if ((int64_t)gy * gx >= (int64_t)1 << 31 || 7 * nodes >= (int64_t)1 << 31 || strips * B >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    if (!vol || !field || !spacing_host || !ws || !vert_offsets || !normals || (reinterpret_cast<uintptr_t>(ws) & 7)) return NPCD_ERR_ARG;
    IsoNormalArgs a{};
    a.vol = vol, a.field = field, a.vert_off = vert_offsets, a.normals = normals, a.level = level;
    a.gx = gx, a.gy = gy, a.gz = gz, a.n = (int)nodes, a.W = (int)strips;
    for (int i = 0; i < 3; ++i) a.spacing[i] = spacing_host[i];
    a.words = reinterpret_cast<const uint32_t*>(static_cast<const int64_t*>(ws) + (int64_t)B * a.W);
    a.wg_verts = reinterpret_cast<const int32_t*>(a.words + (int64_t)B * a.n);
    hipLaunchKernelGGL(iso_normals_kernel, dim3((unsigned)(B * a.W)), dim3(kIsoStrip), 0, static_cast<hipStream_t>(stream), a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
