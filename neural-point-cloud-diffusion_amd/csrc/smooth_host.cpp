// The launches of smooth.hip on the host: the per-lane functions of smooth.h, the code the kernels run, as plain loops over faces, key
// positions and vertices.  A stand-alone program for tests/test_smooth_cpu.py, which holds its output to
// npcd.eval.mesh.mesh_edges_reference and smooth_reference before the kernels run anywhere; it is not part of libnpcd_hip.so.
//
//   smooth_host IN OUT [reverse]
//   IN:  int32 V, F, iterations, flags (1: fixed follows, 2: fix_boundary); float64 lam, mu; float32 vertices [V, 3]; int32 faces [F, 3];
//        uint8 fixed [V] with flag 1
//   OUT: int64 counts [6]; int32 row_start [V + 1], neighbours [D], edges [E, 2], edge_faces [E], edge_forward [E]; uint8
//        boundary_vertex [V]; float32 vertices' [V, 3]; int32 state [V, 3]
// With `reverse` the lanes of every step run in descending order, the prefix sums are taken from the far end (total minus what
// follows) and a vertex sums its row from the far end: integer maxima and sums do not depend on the schedule.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_lanes.h"
#include "smooth.h"

using namespace npcd;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool reverse = argc > 3 && !std::strcmp(argv[3], "reverse");
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[4];
    double factors[2];
    if (std::fread(head, 4, 4, in) != 4 || std::fread(factors, 8, 2, in) != 2) return 2;
    const int64_t V = head[0], F = head[1];
    const int iterations = head[2];
    const bool has_fixed = head[3] & 1, fix_boundary = head[3] & 2;
    const double lam = factors[0], mu = factors[1];
    if (V < 0 || F < 0 || F >= kSmMaxFaces || iterations < 0 || iterations > kSmMaxIterations) return 2;
    if (!(lam > 0.0 && lam <= 1.0) || !(mu >= -1.0 && mu <= 0.0)) return 2;
    std::vector<float> vertices((size_t)V * 3);
    std::vector<int32_t> faces((size_t)F * 3);
    std::vector<uint8_t> fixed(has_fixed ? V : 0);
    if (!read_all(in, vertices) || !read_all(in, faces) || !read_all(in, fixed)) return 2;
    std::fclose(in);
    const LaneOrder order_of{reverse};
    // ---- the edges --------------------------------------------------------------------------------------------------------------------
    const int64_t n = 6 * F, strips = sm_strips(n);
    std::vector<int64_t> keys(n, -7);
    for (int64_t l = 0; l < F; ++l) {          // the keys launch
        const int64_t f = order_of(l, F);
        sm_face_keys(faces.data() + f * 3, V, keys.data() + f * 6);
    }
    std::sort(keys.begin(), keys.end());          // the caller's part
    int64_t counts[kSmCounts] = {0, 0, 0, 0, 0, 0};          // what the unique call zeroes is zero; everything else is poisoned
    std::vector<uint32_t> incl(n, 0xdeadbeefu);
    std::vector<uint64_t> strip_before(strips, 0xdeadbeefdeadbeefull);
    for (int64_t l = 0; l < strips; ++l) {          // the marks launch
        const int64_t s = order_of(l, strips), first = s * kSmStrip, count = std::min<int64_t>(kSmStrip, n - first);
        uint64_t marks[kSmStrip];
        for (int64_t k = 0; k < count; ++k) marks[k] = sm_marks(keys.data(), first + k);
        strip_before[s] = scan_in_place<true>(marks, count, reverse);
        for (int64_t k = 0; k < count; ++k) {
            incl[first + k] = (uint32_t)marks[k] | (uint32_t)(marks[k] >> 32) << 16;
            if (sm_is_last(keys.data(), n, first + k)) counts[kSmCountFaces] = (first + k + 1) / 6;
        }
    }
    counts[kSmCountD] = (int64_t)(scan_in_place<false>(strip_before.data(), strips, reverse) & 0xffffffffu);          // the totals launch
    const int64_t D = counts[kSmCountD], E = D / 2;
    if (D < 0 || D > n || (D & 1)) return 3;
    std::vector<int32_t> row_start(V + 1, D ? -7 : 0), neighbours(D, -7), edges((size_t)E * 2, -7), edge_faces(E, -7), edge_forward(E, -7);
    std::vector<uint8_t> boundary(V, 0);
    if (D) {          // the emit launch
        SmEdges o{row_start.data(), neighbours.data(), edges.data(), edge_faces.data(), edge_forward.data(), boundary.data(), V, D};
        for (int64_t l = 0; l < n; ++l) {
            const int64_t p = order_of(l, n);
            const uint64_t before = strip_before[p / kSmStrip];
            const uint64_t found = sm_emit_lane(keys.data(), n, p, (int64_t)(before & 0xffffffffu) + (incl[p] & 0xffffu),
                                                (int64_t)(before >> 32) + (incl[p] >> 16), o);
            for (int k = 0; k < 4; ++k) counts[kSmCountUsed + k] += (int64_t)((found >> (16 * k)) & 0xffffu);
        }
    }
    // ---- the smoothing ----------------------------------------------------------------------------------------------------------------
    uint32_t a_max = 0;
    for (int64_t l = 0; l < V * 3; ++l) a_max = std::max(a_max, finite_abs_bits(vertices[order_of(l, V * 3)]));          // the measure launch
    const SmRecord poison = {{-7, -7, -7}, 0xdeadbeefu};
    std::vector<SmRecord> state[2] = {std::vector<SmRecord>(V, poison), std::vector<SmRecord>(V, poison)};
    for (int64_t l = 0; l < V; ++l) {          // the quantise launch
        const int64_t i = order_of(l, V);
        state[0][i] = sm_quantise_lane(vertices.data(), i, V, row_start.data(), neighbours.data(), D, fix_boundary ? boundary.data() : nullptr,
                                       has_fixed ? fixed.data() : nullptr, a_max);
    }
    std::vector<float> out(vertices);
    int at = 0;
    if (iterations > 0 && D > 0) {
        for (int it = 0; it < iterations; ++it)
            for (int half = 0; half < (mu == 0.0 ? 1 : 2); ++half, at ^= 1)          // a step launch
                for (int64_t l = 0; l < V; ++l) {
                    const int64_t i = order_of(l, V);
                    state[at ^ 1][i] = sm_step_lane(state[at].data(), i, V, row_start.data(), neighbours.data(), D, half ? mu : lam, reverse);
                }
        std::fill(out.begin(), out.end(), -7.f);
        for (int64_t l = 0; l < V; ++l) {          // the finish launch
            const int64_t i = order_of(l, V);
            sm_finish_lane(vertices.data() + i * 3, state[at][i], a_max, out.data() + i * 3);
        }
    }
    std::vector<int32_t> lattice((size_t)V * 3);
    for (int64_t i = 0; i < V; ++i)
        for (int k = 0; k < 3; ++k) lattice[i * 3 + k] = state[at][i].q[k];
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    const bool ok = std::fwrite(counts, 8, kSmCounts, fo) == (size_t)kSmCounts && write_all(fo, row_start) && write_all(fo, neighbours) &&
                    write_all(fo, edges) && write_all(fo, edge_faces) && write_all(fo, edge_forward) && write_all(fo, boundary) &&
                    write_all(fo, out) && write_all(fo, lattice);
    return std::fclose(fo) == 0 && ok ? 0 : 2;
}
