// The launches of simplify.hip on the host: the per-lane functions of simplify.h, the code the kernels run, as plain loops over
// vertices, bitmap words, clusters and faces.  A stand-alone program for tests/test_simplify_cpu.py, which holds its output to
// npcd.eval.mesh.simplify_reference before the kernels run anywhere; it is not part of libnpcd_hip.so.
//
//   simplify_host IN OUT [reverse]
//   IN:  int32 V, F, C, two_keys; float64 origin [3], cell [3]; int32 dims [3], one int32 of padding; float32 vertices [V, 3];
//        int32 faces [F, 3]; float32 attributes [V, C] if C > 0
//   OUT: int64 V', F'; float32 vertices' [V', 3]; int32 faces' [F', 3]; float32 attributes' [V', C]; int32 vertex_cluster [V];
//        int32 face_source [F']
// With `reverse` the lanes of every step run in descending order and the prefix sums are taken from the far end (total minus what
// follows): integer ORs, maxima and sums do not depend on the schedule.  two_keys sorts the faces by two stable passes, as the wrapper
// does for more than 2^21 clusters.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "host_lanes.h"
#include "simplify.h"

using namespace npcd;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool reverse = argc > 3 && !std::strcmp(argv[3], "reverse");
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[4], dims_pad[4];
    SimpGrid g;
    if (std::fread(head, 4, 4, in) != 4 || std::fread(g.origin, 8, 3, in) != 3 || std::fread(g.cell, 8, 3, in) != 3 ||
        std::fread(dims_pad, 4, 4, in) != 4)
        return 2;
    const int V = head[0], F = head[1], C = head[2];
    const bool two_keys = head[3] != 0;
    for (int a = 0; a < 3; ++a) g.dims[a] = dims_pad[a];
    if (V < 0 || F < 0 || C < 0 || C > kSimpMaxChannels || g.dims[0] < 1 || g.dims[1] < 1 || g.dims[2] < 1) return 2;
    const int64_t cells = simp_cells(g.dims);
    if (cells > kSimpMaxCells) return 2;
    std::vector<float> vertices((size_t)V * 3), attrs((size_t)V * C);
    std::vector<int32_t> faces((size_t)F * 3);
    if (!read_all(in, vertices) || !read_all(in, faces) || !read_all(in, attrs)) return 2;
    std::fclose(in);
    const LaneOrder order_of{reverse};
    const int64_t U = V < cells ? V : cells, words = simp_words(cells), strips = simp_strips(words);
    // what the cluster call zeroes is zero; everything else is poisoned: the steps write every entry they promise
    std::vector<uint64_t> sums((size_t)U * (3 + C), 0);
    std::vector<uint32_t> n(U, 0), bitmap(words, 0), word_before(words, 0xdeadbeefu), strip_before(strips, 0xdeadbeefu), r((size_t)V * 3, 0xdeadbeefu);
    std::vector<int32_t> cluster_key(U, -7), vertex_cluster(V, -7), mapped((size_t)F * 3, -7);
    uint32_t a_max = 0;
    for (int64_t l = 0; l < V; ++l) {          // the mark launch
        const int64_t i = order_of(l, V);
        const int32_t key = simp_mark_lane(vertices.data() + i * 3, g, r.data() + i * 3);
        vertex_cluster[i] = key;
        if (key >= 0) bitmap[key >> 5] |= 1u << (key & 31);
        for (int c = 0; c < C; ++c) a_max = std::max(a_max, finite_abs_bits(attrs[i * C + c]));
    }
    for (int64_t l = 0; l < strips; ++l) {          // the rank launch
        const int64_t s = order_of(l, strips), first = s * kSimpStrip, count = std::min<int64_t>(kSimpStrip, words - first);
        for (int64_t w = 0; w < count; ++w) word_before[first + w] = (uint32_t)popcount32(bitmap[first + w]);
        strip_before[s] = scan_in_place<false>(word_before.data() + first, count, reverse);
    }
    int64_t counts[2] = {scan_in_place<false>(strip_before.data(), strips, reverse), 0};          // the totals launch
    for (int64_t l = 0; l < V; ++l) {          // the accumulate launch
        const int64_t i = order_of(l, V);
        const int32_t key = vertex_cluster[i];
        if (key < 0) continue;
        const int32_t id = simp_cluster_of(key, bitmap.data(), word_before.data(), strip_before.data());
        if (id < 0 || id >= U) return 3;
        vertex_cluster[i] = id;
        cluster_key[id] = key;
        for (int k = 0; k < 3; ++k) sums[(size_t)id * (3 + C) + k] += r[i * 3 + k];
        n[id] += 1;
        for (int c = 0; c < C; ++c) sums[(size_t)id * (3 + C) + 3 + c] += (uint64_t)simp_quantise(attrs[i * C + c], a_max);
    }
    std::vector<int64_t> key_hi(two_keys ? F : 0), key_lo(F), order(F);
    for (int64_t l = 0; l < F; ++l) {          // the faces launch
        const int64_t f = order_of(l, F);
        simp_face_lane(faces.data() + f * 3, vertex_cluster.data(), V, mapped.data() + f * 3);
        simp_face_keys(mapped.data() + f * 3, two_keys ? key_hi.data() + f : nullptr, key_lo.data() + f);
    }
    if (!two_keys && counts[0] > kSimpPackedIds) return 2;
    // the caller's part: a stable order of the keys
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key_lo[x] < key_lo[y]; });
    if (two_keys) std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key_hi[x] < key_hi[y]; });
    std::vector<uint32_t> fword(F, 0), fstrip(simp_strips(F), 0xdeadbeefu);
    for (int64_t l = 0; l < F; ++l) {          // the unique launch
        int64_t face;
        if (simp_keeps(order.data(), order_of(l, F), mapped.data(), F, &face)) fword[face] = 1u;
    }
    for (int64_t l = 0; l < simp_strips(F); ++l) {          // the flags launch
        const int64_t s = order_of(l, simp_strips(F)), first = s * kSimpStrip, count = std::min<int64_t>(kSimpStrip, F - first);
        uint32_t marks[kSimpStrip];
        for (int64_t k = 0; k < count; ++k) marks[k] = fword[first + k] & 1u;
        fstrip[s] = scan_in_place<true>(marks, count, reverse);
        for (int64_t k = 0; k < count; ++k) fword[first + k] = marks[k] << 1 | (fword[first + k] & 1u);
    }
    counts[1] = scan_in_place<false>(fstrip.data(), simp_strips(F), reverse);          // the totals launch
    const int64_t Vp = counts[0], Fp = counts[1];
    if (Vp > U || Fp > F) return 3;
    std::vector<float> vertices_out((size_t)Vp * 3, -7.f), attrs_out((size_t)Vp * C, -7.f);
    std::vector<int32_t> faces_out((size_t)Fp * 3, -7), face_source(Fp, -7);
    for (int64_t l = 0; l < Vp; ++l) {          // the finish launch
        const int64_t id = order_of(l, Vp);
        simp_position(cluster_key[id], sums.data() + (size_t)id * (3 + C), n[id], g, vertices_out.data() + id * 3);
        for (int c = 0; c < C; ++c) attrs_out[id * C + c] = simp_attr_mean((int64_t)sums[(size_t)id * (3 + C) + 3 + c], n[id], a_max);
    }
    for (int64_t l = 0; l < F; ++l) {          // the compact launch
        const int64_t f = order_of(l, F);
        const uint32_t w = fword[f];
        if (!(w & 1u)) continue;
        const int64_t to = (int64_t)fstrip[f / kSimpStrip] + (w >> 1) - 1;
        if (to < 0 || to >= Fp) return 3;
        for (int k = 0; k < 3; ++k) faces_out[to * 3 + k] = mapped[f * 3 + k];
        face_source[to] = (int32_t)f;
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = std::fwrite(counts, 8, 2, out) == 2 && write_all(out, vertices_out) && write_all(out, faces_out) && write_all(out, attrs_out) &&
                    write_all(out, vertex_cluster) && write_all(out, face_source);
    return std::fclose(out) == 0 && ok ? 0 : 2;
}
