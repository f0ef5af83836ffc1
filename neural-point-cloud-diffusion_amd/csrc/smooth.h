// The edges of a triangle mesh and Taubin smoothing on an integer lattice: the per-lane arithmetic of csrc/smooth.hip,
// written once for the device and the host.  The kernels run these functions one lane per face, key position or vertex; the stand-alone
// program csrc/smooth_host.cpp runs them as plain loops (tests/test_smooth_cpu.py): this header includes nothing of HIP.  All float64
// arithmetic is as written -- the file is compiled without FMA contraction (build.py) -- and the divisions are the correctly rounded ones.
//
//   Face      valid if its three indices lie in [0, V) and differ pairwise; nothing is read through any other face.
//   Pairs     a valid face (i, j, k) gives i->j, j->k, k->i (forward) and the three reversed (backward).  The key of a->b is
//             a 2^31 + b < 2^62; what is sorted is key 2 + backward < 2^63, so a run of one key keeps how its faces traverse it.  A
//             face that is not valid gives six times INT64_MAX: after every valid one.
//   Heads     in the ascending order of the 6F sort keys a position is a head if its key is valid and differs from the key before it.
//             The heads are the distinct keys, D of them; the heads with a < b are the edges, E = D / 2 of them.
//   Emit      the head of rank r writes neighbours[r] = b and, where its source a is larger than the source before it, row_start[v] = r
//             for the vertices v between that source (excluded) and a (included); the last valid position writes row_start[v] = D for
//             the v above its source.  A head with a < b walks its run: the length is edge_faces, the even sort keys edge_forward.
//   Lattice   A = the largest finite |coordinate| (an integer maximum on the bits), e = floor(log2 A) from the exponent of
//             float64(A), q = rint(float64(x) 2^(29 - e)), |q| <= 2^30.  A vertex with a coordinate that is not finite is lost.
//   Step      S = the integer sum of q over the neighbours that are not lost, d their number:
//             q' = clamp(q + rint(f (float64(S) / float64(d) - float64(q))), -(2^31 - 1), 2^31 - 1) per axis.
//   Finish    fp32 of float64(q) 2^(e - 29) for a vertex that moves, the input bits for every other.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bits.h"

namespace npcd {

// lanes per workgroup of every launch; key positions per strip of the two-level prefix sums: one entry per lane
constexpr int kSmThreads = 256;
constexpr int kSmStrip = 256;
constexpr int64_t kSmMaxVertices = (int64_t)1 << 31;          // V below it: an index is 31 bits of a key
constexpr int64_t kSmMaxFaces = (int64_t)1 << 28;             // F below it: 6F positions are counted in 32 bits
constexpr int kSmMaxIterations = 1000;
constexpr int64_t kSmNoKey = INT64_MAX;
constexpr int64_t kSmClamp = 2147483647;                      // |q| stays at most 2^31 - 1
constexpr uint32_t kSmLost = 1u, kSmMoves = 2u;               // the flag word of a record
// the slots of counts [6] int64
enum { kSmCountD = 0, kSmCountFaces, kSmCountUsed, kSmCountBoundary, kSmCountNonManifold, kSmCountMisoriented, kSmCounts };

// the state of one vertex: one 16-byte load says where a neighbour is and whether it counts
struct alignas(16) SmRecord {
    int32_t q[3];
    uint32_t flag;
};

NPCD_HD int64_t sm_strips(int64_t entries) { return (entries + kSmStrip - 1) / kSmStrip; }

// ---- one face of the keys launch ------------------------------------------------------------------------------------------------------
NPCD_HD bool sm_face_valid(const int32_t* f, int64_t V) {
    for (int k = 0; k < 3; ++k)
        if (f[k] < 0 || f[k] >= V) return false;
    return f[0] != f[1] && f[1] != f[2] && f[0] != f[2];
}
NPCD_HD int64_t sm_sort_key(int32_t a, int32_t b, int backward) { return (((((int64_t)a) << 31) | (int64_t)b) << 1) | (int64_t)backward; }
// keys [6]: the three forward pairs, then the three backward ones
NPCD_HD void sm_face_keys(const int32_t* f, int64_t V, int64_t* keys) {
    if (!sm_face_valid(f, V)) {
        for (int k = 0; k < 6; ++k) keys[k] = kSmNoKey;
        return;
    }
    for (int k = 0; k < 3; ++k) {
        const int32_t a = f[k], b = f[k == 2 ? 0 : k + 1];
        keys[k] = sm_sort_key(a, b, 0), keys[3 + k] = sm_sort_key(b, a, 1);
    }
}
NPCD_HD int64_t sm_pair(int64_t sort_key) { return sort_key >> 1; }
NPCD_HD int64_t sm_source(int64_t sort_key) { return sort_key >> 32; }
NPCD_HD int64_t sm_target(int64_t sort_key) { return (sort_key >> 1) & 0x7fffffff; }

// ---- one position of the sorted keys -------------------------------------------------------------------------------------------------
NPCD_HD bool sm_is_head(const int64_t* keys, int64_t p) {
    return keys[p] != kSmNoKey && (p == 0 || sm_pair(keys[p - 1]) != sm_pair(keys[p]));
}
// 1 for a head, 2^32 more for a head with a < b: both prefix sums in one
NPCD_HD uint64_t sm_marks(const int64_t* keys, int64_t p) {
    if (!sm_is_head(keys, p)) return 0;
    return 1u + (sm_source(keys[p]) < sm_target(keys[p]) ? (uint64_t)1 << 32 : 0);
}
// the last valid position holds 6 F_v - 1
NPCD_HD bool sm_is_last(const int64_t* keys, int64_t n, int64_t p) { return keys[p] != kSmNoKey && (p == n - 1 || keys[p + 1] == kSmNoKey); }

struct SmEdges {          // the outputs of the emit launch
    int32_t *row_start, *neighbours, *edges, *edge_faces, *edge_forward;          // [V + 1], [D], [E, 2], [E], [E]
    uint8_t* boundary_vertex;                                                     // [V], zero before
    int64_t V, D;
};
// position p of n sorted keys; heads, edges: the inclusive counts of sm_marks up to and including p.  -> used | boundary 2^16 |
// non-manifold 2^32 | misoriented 2^48, each 0 or 1.  Every index is held to its array: a key that is not this mesh's writes nothing.
NPCD_HD uint64_t sm_emit_lane(const int64_t* keys, int64_t n, int64_t p, int64_t heads, int64_t edges, const SmEdges& o) {
    const int64_t key = keys[p];
    if (key == kSmNoKey) return 0;
    const int64_t a = sm_source(key), b = sm_target(key);
    if (a < 0 || a >= o.V || b >= o.V) return 0;          // (cannot be)
    uint64_t counts = 0;
    if (sm_is_head(keys, p)) {
        const int64_t r = heads - 1;
        if (r < 0 || r >= o.D) return 0;          // (cannot be)
        o.neighbours[r] = (int32_t)b;
        const int64_t before = p == 0 ? -1 : sm_source(keys[p - 1]);
        if (before < a) {          // the first key of its row: the rows of the unused vertices before it are empty
            for (int64_t v = before < 0 ? 0 : before + 1; v <= a; ++v) o.row_start[v] = (int32_t)r;
            counts |= 1u;
        }
        if (a < b) {
            int32_t faces = 0, forward = 0;
            for (int64_t j = p; j < n && keys[j] != kSmNoKey && sm_pair(keys[j]) == sm_pair(key); ++j) faces += 1, forward += (int32_t)(~keys[j] & 1);
            const int64_t e = edges - 1;
            if (e >= 0 && e < o.D / 2) {
                o.edges[e * 2] = (int32_t)a, o.edges[e * 2 + 1] = (int32_t)b;
                o.edge_faces[e] = faces, o.edge_forward[e] = forward;
            }
            if (faces == 1) {
                o.boundary_vertex[a] = 1, o.boundary_vertex[b] = 1;          // every writer stores the same byte
                counts |= (uint64_t)1 << 16;
            }
            if (faces >= 3) counts |= (uint64_t)1 << 32;
            if (faces == 2 && forward != 1) counts |= (uint64_t)1 << 48;
        }
    }
    if (sm_is_last(keys, n, p))
        for (int64_t v = a + 1; v <= o.V; ++v) o.row_start[v] = (int32_t)o.D;
    return counts;
}

// ---- the lattice ---------------------------------------------------------------------------------------------------------------------
NPCD_HD bool sm_lost(const float* v) { return !(is_finite(v[0]) && is_finite(v[1]) && is_finite(v[2])); }
// 29 - floor(log2 A) for A > 0: A maps into [2^29, 2^30), |q| <= 2^30
NPCD_HD int sm_shift(uint32_t a_max_bits) { return 29 - floor_log2(bits_float(a_max_bits)); }
// the row of vertex i in the adjacency, held to [0, D]
NPCD_HD void sm_row(const int32_t* row_start, int64_t i, int64_t D, int64_t* begin, int64_t* end) {
    const int64_t lo = row_start[i], hi = row_start[i + 1];
    *begin = lo < 0 ? 0 : lo > D ? D : lo;
    *end = hi < *begin ? *begin : hi > D ? D : hi;
}
// one vertex of the quantise launch: its place on the lattice, lost or not, and whether it moves.  boundary and fixed may be null.
NPCD_HD SmRecord sm_quantise_lane(const float* vertices, int64_t i, int64_t V, const int32_t* row_start, const int32_t* neighbours,
                                       int64_t D, const uint8_t* boundary, const uint8_t* fixed, uint32_t a_max_bits) {
    SmRecord r = {{0, 0, 0}, 0u};
    const float* v = vertices + i * 3;
    if (sm_lost(v)) {
        r.flag = kSmLost;
        return r;
    }
    if (a_max_bits) {
        const double scale = pow2(sm_shift(a_max_bits));
        for (int k = 0; k < 3; ++k) r.q[k] = (int32_t)rint((double)v[k] * scale);
    }
    if ((fixed && fixed[i]) || (boundary && boundary[i])) return r;
    int64_t begin, end;
    sm_row(row_start, i, D, &begin, &end);
    for (int64_t j = begin; j < end; ++j) {
        const int64_t nb = neighbours[j];
        if (nb >= 0 && nb < V && !sm_lost(vertices + nb * 3)) {
            r.flag = kSmMoves;
            break;
        }
    }
    return r;
}
// one vertex of a step launch: the old state in `state`, -> its new record
NPCD_HD SmRecord sm_step_lane(const SmRecord* state, int64_t i, int64_t V, const int32_t* row_start, const int32_t* neighbours, int64_t D,
                                   double factor, bool from_the_end = false) {
    SmRecord own = state[i];
    if (!(own.flag & kSmMoves)) return own;
    int64_t begin, end, sum[3] = {0, 0, 0}, degree = 0;
    sm_row(row_start, i, D, &begin, &end);
    for (int64_t t = begin; t < end; ++t) {
        const int64_t nb = neighbours[from_the_end ? end - 1 - (t - begin) : t];
        if (nb < 0 || nb >= V) continue;          // (cannot be)
        const SmRecord other = state[nb];
        if (other.flag & kSmLost) continue;
        sum[0] += other.q[0], sum[1] += other.q[1], sum[2] += other.q[2];
        degree += 1;
    }
    if (degree == 0) return own;          // (cannot be: it moves)
    for (int k = 0; k < 3; ++k) {
        const double mean = (double)sum[k] / (double)degree;
        const int64_t q = (int64_t)own.q[k] + (int64_t)rint(factor * (mean - (double)own.q[k]));
        own.q[k] = (int32_t)(q < -kSmClamp ? -kSmClamp : q > kSmClamp ? kSmClamp : q);
    }
    return own;
}
// one vertex of the finish launch
NPCD_HD void sm_finish_lane(const float* in, const SmRecord& r, uint32_t a_max_bits, float* out) {
    if (!(r.flag & kSmMoves) || a_max_bits == 0) {
        for (int k = 0; k < 3; ++k) out[k] = bits_float(float_bits(in[k]));
        return;
    }
    const double quantum = pow2(-sm_shift(a_max_bits));
    for (int k = 0; k < 3; ++k) out[k] = (float)((double)r.q[k] * quantum);
}

}  // namespace npcd
