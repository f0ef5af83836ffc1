// Connected components of the nodes of a density volume above a level: the labelling under
// npcd.hip.components (label_components, filter_components), which drops floaters from a volume before it is meshed.
//
//   vol [B, gz, gy, gx] fp32, x fastest, as csrc/isosurface.hip reads it: inside iff f > level, adjacent along the seven edge types.
//   labels [B, n] int32: -1 outside, otherwise the smallest node index of the node's component, local to its volume.
//   sizes  [B, n] int32: the number of nodes of a component at its root node, 0 everywhere else.
//
// The union-find, its invariant and the bound of every loop are stated in components.h, which holds the phases themselves; this file
// gives them their atomics and their launches.
//   tile:   a workgroup owns a brick of 16 x 8 x 8 nodes, four to a lane.  Its 1,024 labels sit in LDS; the edges inside the brick are
//           joined with ds integer minima, and every node's root goes to ws as a node index of the volume -- a forest with one tree per
//           piece of a component inside a brick.  The pieces' nodes are counted in LDS as well and go to sizes at the pieces' roots.
//   merge:  the same grid; a node on an upper face of its brick joins the two trees at the ends of every edge that leaves the brick,
//           always the larger root under the smaller, with agent-scope integer minima on ws.  A lane may read an entry as another
//           workgroup left it some time ago: any value an entry ever held is a node of the component below the entry's index, so
//           the walk stays correct (components.h); the minima themselves are atomic chip-wide.
//   final:  one node per lane in node order, after the forest is complete: the label is the root, and the root of a piece that is not
//           its component's adds the piece's nodes to sizes[root] with one integer atomic -- one addition per piece, so a component of
//           a million nodes is not a million additions to one word.
// Three launches on the caller's stream, no host synchronisation, no allocation, no float atomics.
//
// Bounds.  A brick node the volume does not have reads nothing, counts as outside and writes nothing; an edge is followed only to a
// node of the volume; local indices stay below 1,024 because an edge that would leave the brick is left to the merge phase.
// gz gy gx < 2^31 (checked), so node indices are ints; the offset of a volume in the batch is 64 bits.
#include "common.h"
#include "components.h"

namespace npcd {

template <int SCOPE>
struct CcAtomic {
    static __device__ __forceinline__ int load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
    static __device__ __forceinline__ int fetch_min(int32_t* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE); }
    static __device__ __forceinline__ void add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE); }
};
using CcLds = CcAtomic<__HIP_MEMORY_SCOPE_WORKGROUP>;
using CcGlobal = CcAtomic<__HIP_MEMORY_SCOPE_AGENT>;

struct CcArgs {
    const float* vol;          // [B, n]
    int32_t* parent;           // [B, n], the workspace
    int32_t *labels, *sizes;          // [B, n]
    float level;
    CcGrid g;
    int strips;                // workgroups of the final phase per volume
};

__global__ __launch_bounds__(kCcThreads) void cc_tile_kernel(CcArgs a) {
    __shared__ int32_t local[kCcBrickNodes], count[kCcBrickNodes];
    const int b = blockIdx.x / a.g.bricks, brick = blockIdx.x - b * a.g.bricks;
    const int64_t base = (int64_t)b * a.g.n;
#pragma unroll
    for (int k = 0; k < kCcNodesPerLane; ++k) cc_tile_load(a.g, a.vol + base, a.level, brick, threadIdx.x + k * kCcThreads, local, count);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcNodesPerLane; ++k) cc_tile_link<CcLds>(threadIdx.x + k * kCcThreads, local);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcNodesPerLane; ++k) cc_tile_count<CcLds>(threadIdx.x + k * kCcThreads, local, count);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcNodesPerLane; ++k)
        cc_tile_store(a.g, brick, threadIdx.x + k * kCcThreads, local, count, a.parent + base, a.sizes + base);
}

__global__ __launch_bounds__(kCcThreads) void cc_merge_kernel(CcArgs a) {
    const int b = blockIdx.x / a.g.bricks, brick = blockIdx.x - b * a.g.bricks;
#pragma unroll
    for (int k = 0; k < kCcNodesPerLane; ++k)
        cc_merge_node<CcGlobal>(a.g, brick, threadIdx.x + k * kCcThreads, a.parent + (int64_t)b * a.g.n);
}

__global__ __launch_bounds__(kCcThreads) void cc_final_kernel(CcArgs a) {
    const int b = blockIdx.x / a.strips, node = (blockIdx.x - b * a.strips) * kCcThreads + threadIdx.x;
    const int64_t base = (int64_t)b * a.g.n;
    if (node < a.g.n) cc_final_node<CcGlobal>(a.parent + base, node, a.labels + base, a.sizes + base);
}

static inline int cc_check(int B, int gz, int gy, int gx, CcArgs* a) {
    if (B <= 0 || gz < 2 || gy < 2 || gx < 2) return NPCD_ERR_ARG;
    const int64_t slab = (int64_t)gy * gx;
    if (slab >= (int64_t)1 << 31 || slab * gz >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    a->g = cc_grid(gz, gy, gx);
    a->strips = (a->g.n + kCcThreads - 1) / kCcThreads;
    if ((int64_t)B * a->g.bricks >= (int64_t)1 << 31 || (int64_t)B * a->strips >= (int64_t)1 << 31) return NPCD_ERR_UNSUPPORTED;
    return NPCD_OK;
}

}  // namespace npcd

using namespace npcd;

extern "C" int64_t npcd_components_ws_bytes(int B, int gz, int gy, int gx) {
    CcArgs a{};
    const int rc = cc_check(B, gz, gy, gx, &a);
    return rc != NPCD_OK ? rc : (int64_t)B * a.g.n * 4;
}

extern "C" int npcd_components_label(const float* vol, int B, int gz, int gy, int gx, float level, void* ws, int32_t* labels, int32_t* sizes,
                                     void* stream) {
    CcArgs a{};
    const int rc = cc_check(B, gz, gy, gx, &a);
    if (rc != NPCD_OK) return rc;
    if (!vol || !ws || !labels || !sizes) return NPCD_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(vol) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(labels) |
         reinterpret_cast<uintptr_t>(sizes)) & 3)
        return NPCD_ERR_ARG;
    a.vol = vol, a.parent = static_cast<int32_t*>(ws), a.labels = labels, a.sizes = sizes, a.level = level;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(B * a.g.bricks)), dim3(kCcThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)(B * a.g.bricks)), dim3(kCcThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cc_final_kernel, dim3((unsigned)(B * a.strips)), dim3(kCcThreads), 0, s, a);
    NPCD_HIP_CHECK(hipGetLastError());
    return NPCD_OK;
}
