// Vertex clustering of a triangle mesh: the per-lane arithmetic of csrc/simplify.hip, written once for the device and
// the host.  The kernels run these functions one lane per vertex, bitmap word, cluster or face; the stand-alone program
// csrc/simplify_host.cpp runs them as plain loops (tests/test_simplify_cpu.py): this header includes nothing of HIP.  All float64
// arithmetic is as written -- the file is compiled without FMA contraction (build.py) -- and the divisions are the correctly rounded ones.
//
//   Cell      u = (float64(v) - origin) / cell per axis; a vertex with a u that is not finite is lost (key -1).  c = clamp(floor(u), 0,
//             dims - 1), key = (cz dims_y + cy) dims_x + cx < 2^30, r = clamp(floor((u - c) 2^32), 0, 2^32 - 1): the place inside the cell
//             as an integer.
//   Cluster   the rank of the key among the occupied cells: a bitmap of the cells, 32 to a word, the exclusive sums of the words'
//             popcounts (inside strips of kSimpStrip words, then over the strip totals), plus the set bits below the cell's own.
//   Sums      S = the integer sums of r over the cluster, n the count: position = origin + cell (c + (float64(S) / float64(n)) 2^-32).
//   Attributes  A = the largest finite |a| of the call (an integer maximum on the bits), e = floor(log2 A) from the exponent of
//             float64(A), q = rint(float64(a) 2^(30 - e)) (exact product, |q| <= 2^31; a value that is not finite counts as 0), summed
//             as signed 64-bit integers: mean = (float64(sum) / float64(n)) 2^(e - 30).
//   Faces     a face maps to its corners' clusters; it is valid if every index lies in [0, V), no corner is lost and the three clusters
//             differ.  Its sort key holds the sorted triple; among valid faces with the same sorted triple the lowest index stays.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bits.h"

namespace npcd {

// lanes per workgroup of every launch; bitmap words (and face flags) per strip of the two-level prefix sums: one entry per lane
constexpr int kSimpThreads = 256;
constexpr int kSimpStrip = 256;
constexpr int kSimpMaxChannels = 16;
constexpr int64_t kSimpMaxCells = (int64_t)1 << 30;
// one packed key holds a sorted triple of cluster ids below 2^21
constexpr int64_t kSimpPackedIds = (int64_t)1 << 21;
constexpr int64_t kSimpNoKey = INT64_MAX;          // the key of a face that is not valid: after every valid one

struct SimpGrid {
    double origin[3], cell[3];
    int dims[3];
};

NPCD_HD int64_t simp_cells(const int* dims) { return (int64_t)dims[0] * dims[1] * dims[2]; }
NPCD_HD int64_t simp_words(int64_t cells) { return (cells + 31) / 32; }
NPCD_HD int64_t simp_strips(int64_t entries) { return (entries + kSimpStrip - 1) / kSimpStrip; }

// ---- one vertex of the mark launch ---------------------------------------------------------------------------------------------------
// -> the key of the vertex's cell, -1 for a lost vertex (r is then 0); r [3] the place inside the cell
NPCD_HD int32_t simp_mark_lane(const float* v, const SimpGrid& g, uint32_t* r) {
    int c[3];
    bool lost = false;
    for (int a = 0; a < 3; ++a) {
        const double u = ((double)v[a] - g.origin[a]) / g.cell[a];
        r[a] = 0, c[a] = 0;
        if (!(fabs(u) < INFINITY)) {
            lost = true;
            continue;
        }
        const double fl = floor(u), top = (double)(g.dims[a] - 1);
        c[a] = !(fl > 0.0) ? 0 : fl >= top ? g.dims[a] - 1 : (int)fl;
        const double t = floor((u - (double)c[a]) * 4294967296.0);
        r[a] = !(t > 0.0) ? 0u : t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
    }
    if (lost) {
        r[0] = r[1] = r[2] = 0;
        return -1;
    }
    return (int32_t)(((int64_t)c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0]);
}

// ---- attributes ------------------------------------------------------------------------------------------------------------------------
// 30 - floor(log2 A) for A > 0: A maps into [2^30, 2^31), |q| <= 2^31
NPCD_HD int simp_attr_shift(uint32_t a_max_bits) { return 30 - floor_log2(bits_float(a_max_bits)); }
NPCD_HD int64_t simp_quantise(float a, uint32_t a_max_bits) {
    if (a_max_bits == 0 || finite_abs_bits(a) == 0) return 0;
    return (int64_t)rint((double)a * pow2(simp_attr_shift(a_max_bits)));
}
NPCD_HD float simp_attr_mean(int64_t sum, uint32_t n, uint32_t a_max_bits) {
    if (a_max_bits == 0) return 0.f;
    return (float)(((double)sum / (double)n) * pow2(-simp_attr_shift(a_max_bits)));
}

// ---- the rank of a cell ---------------------------------------------------------------------------------------------------------------
// word_before: per bitmap word the set bits of its strip before it; strip_before: per strip the set bits before it
NPCD_HD int32_t simp_cluster_of(int32_t key, const uint32_t* bitmap, const uint32_t* word_before, const uint32_t* strip_before) {
    const int32_t w = key >> 5;
    return (int32_t)(strip_before[w / kSimpStrip] + word_before[w] + (uint32_t)popcount32(bitmap[w] & ((1u << (key & 31)) - 1u)));
}

// ---- one cluster of the finish launch -------------------------------------------------------------------------------------------------
NPCD_HD void simp_position(int32_t key, const uint64_t* S, uint32_t n, const SimpGrid& g, float* out) {
    const int c[3] = {key % g.dims[0], (key / g.dims[0]) % g.dims[1], key / g.dims[0] / g.dims[1]};
    for (int a = 0; a < 3; ++a) out[a] = (float)(g.origin[a] + g.cell[a] * ((double)c[a] + ((double)S[a] / (double)n) * 0x1p-32));
}

// ---- one face --------------------------------------------------------------------------------------------------------------------------
// the clusters of the corners to m [3], corner order kept; false (and m = -1, -1, -1) for a face that goes: an index outside [0, V) --
// nothing is read through it --, a lost corner or two corners in one cluster
NPCD_HD bool simp_face_lane(const int32_t* face, const int32_t* vertex_cluster, int V, int32_t* m) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const int i = face[k];
        m[k] = i >= 0 && i < V ? vertex_cluster[i] : -1;
        ok = ok && m[k] >= 0;
    }
    ok = ok && m[0] != m[1] && m[1] != m[2] && m[0] != m[2];
    if (!ok) m[0] = m[1] = m[2] = -1;
    return ok;
}
NPCD_HD void simp_sorted(const int32_t* m, int32_t* s) {
    int32_t a = m[0], b = m[1], c = m[2], t;
    if (a > b) t = a, a = b, b = t;
    if (b > c) t = b, b = c, c = t;
    if (a > b) t = a, a = b, b = t;
    s[0] = a, s[1] = b, s[2] = c;
}
// the sort keys of a mapped face (m[0] < 0: not valid): one packed key (key_hi null; every id below 2^21) or two
NPCD_HD void simp_face_keys(const int32_t* m, int64_t* key_hi, int64_t* key_lo) {
    if (m[0] < 0) {
        *key_lo = kSimpNoKey;
        if (key_hi) *key_hi = kSimpNoKey;
        return;
    }
    int32_t s[3];
    simp_sorted(m, s);
    if (key_hi) *key_hi = s[0], *key_lo = ((int64_t)s[1] << 32) | s[2];
    else *key_lo = ((int64_t)s[0] << 42) | ((int64_t)s[1] << 21) | s[2];
}
// position i of the sorted order: does face order[i] stay?  It is valid and the face before it in the order is not one of the same
// sorted triple (the sort is stable: the first of a run is its lowest index).  An entry of `order` outside [0, F) is not followed.
NPCD_HD bool simp_keeps(const int64_t* order, int64_t i, const int32_t* mapped, int64_t F, int64_t* face) {
    *face = order[i];
    if (*face < 0 || *face >= F) return false;
    const int32_t* m = mapped + *face * 3;
    if (m[0] < 0) return false;
    if (i == 0) return true;
    const int64_t before = order[i - 1];
    if (before < 0 || before >= F) return true;
    const int32_t* p = mapped + before * 3;
    if (p[0] < 0) return true;
    int32_t s[3], t[3];
    simp_sorted(m, s), simp_sorted(p, t);
    return s[0] != t[0] || s[1] != t[1] || s[2] != t[2];
}

}  // namespace npcd
