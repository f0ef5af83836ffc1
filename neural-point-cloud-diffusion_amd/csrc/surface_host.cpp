// The launches of surface.hip on the host: the per-lane functions of surface.h, the code the kernels run, as plain loops over tile slots,
// lanes and samples.  A stand-alone program for tests/test_surface_sampling_cpu.py, which holds its output to
// npcd.eval.mesh.surface_sample_reference before the kernels run anywhere; it is not part of libnpcd_hip.so.
//
//   surface_host IN OUT [reverse]
//   IN:  int32 B, S, C, normals_mode, V_total, F_total; int32 vert_offsets [B + 1], face_offsets [B + 1]; float32 vertices [V_total, 3];
//        int32 faces [F_total, 3]; float32 u [B, S, 3]; float32 vertex normals [V_total, 3] if normals_mode is 2; float32 attributes
//        [V_total, C] if C > 0
//   OUT: float64 area [B]; float32 points [B, S, 3]; int32 face [B, S]; float32 normals [B, S, 3] if normals_mode; float32 attributes
//        [B, S, C] if C > 0
// With `reverse` the slots, the lanes of every step and the samples run in descending order, and the sums inside a tile and over the
// tiles are taken from the far end (total minus what follows): integer sums and maxima do not depend on the schedule.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_lanes.h"
#include "surface.h"

using namespace npcd;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const bool reverse = argc > 3 && !std::strcmp(argv[3], "reverse");
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[6];
    if (std::fread(head, 4, 6, in) != 6) return 2;
    const int B = head[0], S = head[1], C = head[2], mode = head[3], V_total = head[4], F_total = head[5];
    if (B < 1 || S < 1 || C < 0 || C > kSurfMaxChannels || mode < 0 || mode > 2 || V_total < 0 || F_total < 0) return 2;
    std::vector<int32_t> vert_off(B + 1), face_off(B + 1), faces((size_t)F_total * 3);
    std::vector<float> vertices((size_t)V_total * 3), u((size_t)B * S * 3), vnormals(mode == 2 ? (size_t)V_total * 3 : 0), attrs((size_t)V_total * C);
    if (!read_all(in, vert_off) || !read_all(in, face_off) || !read_all(in, vertices) || !read_all(in, faces) || !read_all(in, u) ||
        !read_all(in, vnormals) || !read_all(in, attrs))
        return 2;
    std::fclose(in);
    const int slots = (int)surf_slots(B, F_total);
    const LaneOrder order{reverse};
    // poisoned: the steps write every entry they promise
    std::vector<float> d(F_total, -7.f);
    std::vector<uint32_t> d_max(B, 0);
    std::vector<uint64_t> local(F_total, ~(uint64_t)0), tiles(slots, ~(uint64_t)0), mesh_W(B, ~(uint64_t)0);
    std::vector<double> area(B, -7.0);
    for (int pass = 0; pass < 2; ++pass)          // the measure launch, then the quantise launch
        for (int w = 0; w < slots; ++w) {
            const int slot = order(w, slots), b = surf_slot_member(face_off.data(), B, slot);
            const SurfSpan fs = surf_span(face_off.data(), b, F_total), vs = surf_span(vert_off.data(), b, V_total);
            const int64_t tile = slot - surf_tile_base(face_off[b], b);
            if (tile < 0 || tile >= surf_tiles(fs.count)) continue;
            uint64_t w_tile[kSurfTile];
            for (int l = 0; l < kSurfTile; ++l) {
                const int lane = order(l, kSurfTile);
                const int64_t i = tile * kSurfTile + lane;
                w_tile[lane] = 0;
                if (i >= fs.count) continue;
                if (pass == 0) {
                    const uint32_t bits = surf_measure_lane(vertices.data() + (size_t)vs.first * 3, faces.data() + (size_t)fs.first * 3, vs.count,
                                                            (int)i, d.data() + fs.first);
                    if (bits > d_max[b]) d_max[b] = bits;
                } else {
                    w_tile[lane] = surf_quantise(d[fs.first + i], d_max[b]);
                }
            }
            if (pass == 0) continue;
            tiles[slot] = scan_in_place<true>(w_tile, kSurfTile, reverse);
            for (int l = 0; l < kSurfTile; ++l)
                if (tile * kSurfTile + l < fs.count) local[fs.first + tile * kSurfTile + l] = w_tile[l];
        }
    for (int w = 0; w < B; ++w) {          // the tiles launch
        const int b = order(w, B);
        const SurfSpan fs = surf_span(face_off.data(), b, F_total);
        mesh_W[b] = scan_in_place<true>(tiles.data() + surf_tile_base(fs.first, b), surf_tiles(fs.count), reverse);
        area[b] = surf_area(mesh_W[b], d_max[b]);
    }
    std::vector<float> points((size_t)B * S * 3, -7.f), normals(mode ? (size_t)B * S * 3 : 0, -7.f), attrs_out((size_t)B * S * C, -7.f);
    std::vector<int32_t> face((size_t)B * S, -7);
    for (int w = 0; w < B; ++w) {          // the sample launch
        const int b = order(w, B);
        const SurfSpan fs = surf_span(face_off.data(), b, F_total), vs = surf_span(vert_off.data(), b, V_total);
        SurfMesh m;
        m.vertices = vertices.data() + (size_t)vs.first * 3, m.faces = faces.data() + (size_t)fs.first * 3;
        m.local = local.data() + fs.first, m.tiles = tiles.data() + surf_tile_base(fs.first, b);
        m.vnormals = mode == 2 ? vnormals.data() + (size_t)vs.first * 3 : nullptr;
        m.attrs = C ? attrs.data() + (size_t)vs.first * C : nullptr;
        m.V = vs.count, m.F = fs.count, m.C = C, m.normals_mode = mode, m.W = mesh_W[b];
        for (int j = 0; j < S; ++j) {
            const size_t row = (size_t)b * S + order(j, S);
            SurfRow o;
            o.point = points.data() + row * 3, o.face = face.data() + row;
            o.normal = mode ? normals.data() + row * 3 : nullptr, o.attr = C ? attrs_out.data() + row * C : nullptr;
            surf_sample_row(m, u.data() + row * 3, o);
        }
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = write_all(out, area) && write_all(out, points) && write_all(out, face) && write_all(out, normals) && write_all(out, attrs_out);
    return std::fclose(out) == 0 && ok ? 0 : 2;
}
