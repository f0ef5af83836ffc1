// What the stand-alone host programs (surface_host.cpp, simplify_host.cpp, smooth_host.cpp, components_host.cpp, mesh_distance_host.cpp,
// raycast_host.cpp, crossings_host.cpp) share: whole-array file I/O, the order in which a loop stands in for the lanes of a launch, the prefix sums that
// stand in for the kernels' scans and, for the mesh query programs, the head and tail of their files, the boxes launch and the tile
// walk of csrc/tile_walk.h over the same Query policies.  Host only; not part of libnpcd_hip.so.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mesh_tiles.h"

namespace npcd {

template <class T>
bool read_all(FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T>
bool write_all(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

// step i of `count` -> the lane, workgroup or entry it runs: ascending, or with `reverse` descending
struct LaneOrder {
    bool reverse;
    int64_t operator()(int64_t i, int64_t count) const { return reverse ? count - 1 - i : i; }
};

// x [n] to its prefix sums in place -- INCLUSIVE: up to and including the entry itself, else before it -- forward, or with `reverse`
// from the far end: the total minus what follows.  -> the total
template <bool INCLUSIVE, class T>
T scan_in_place(T* x, int64_t n, bool reverse) {
    T total = 0;
    if (!reverse) {
        for (int64_t i = 0; i < n; ++i) {
            const T own = x[i];
            x[i] = INCLUSIVE ? total + own : total;
            total += own;
        }
        return total;
    }
    for (int64_t i = n - 1; i >= 0; --i) total += x[i];
    T after = 0;
    for (int64_t i = n - 1; i >= 0; --i) {
        const T own = x[i];
        x[i] = INCLUSIVE ? total - after : total - after - own;
        after += own;
    }
    return total;
}

// ---- the mesh query programs: PROGRAM IN OUT [reverse] [wave] ----------------------------------------------------------------------------
// the head of an input file: int32 N (queries), V, F
inline bool read_head(FILE* in, int64_t* N, int64_t* V, int64_t* F) {
    int32_t head[3];
    if (std::fread(head, 4, 3, in) != 3) return false;
    *N = head[0], *V = head[1], *F = head[2];
    return *N >= 0 && *V >= 0 && *F >= 0 && *F < kMdMaxFaces;
}

// the workspace that the boxes launch leaves: whatever no lane writes stays poisoned
struct HostTiles {
    int64_t F, tiles;
    std::vector<MdCorner> corners;
    std::vector<MdBox> boxes;
    HostTiles(const std::vector<float>& vertices, int64_t V, const std::vector<int32_t>& faces, int64_t F_, LaneOrder order)
        : F(F_), tiles(md_tiles(F_)), corners((size_t)tiles * kMdTile * 3, MdCorner{-7.f, -7.f, -7.f, -7.f}), boxes(tiles) {
        for (int64_t l = 0; l < tiles * kMdTile; ++l) {
            const int64_t f = order(l, tiles * kMdTile);
            md_corners_lane(vertices.data(), V, faces.data(), F, f, corners.data() + f * 3);
        }
        for (int64_t t = 0; t < tiles; ++t) boxes[t] = md_box_of(corners.data() + t * kMdTile * 3, kMdTile * 3);
    }
    const MdCorner* face(int64_t f) const { return corners.data() + f * 3; }
};

// tile_eval (tile_walk.h): every lane of a wave takes the faces of tile t, those below F
template <class Query>
void host_tile_eval(const Query* q, int lanes, const HostTiles& m, int64_t t, typename Query::State* state) {
    for (int l = 0; l < lanes; ++l)
        for (int64_t f = t * kMdTile; f < m.F && f < (t + 1) * kMdTile; ++f) q[l].face(m.face(f), (int32_t)f, &state[l]);
}

// tile_walk<Query, true> (tile_walk.h) for all queries, in waves of W consecutive ones; `order` gives the tile of each step of the
// walk, finish(i, best, best_face) stores what the kernel stores for query i.  A tile is evaluated, by every lane, if any lane asks
// for it.  A wave of one lane scans one box at a time: it judges every box with its best of the moment, which is what these programs
// count without `wave`.  -> the (wave, tile) pairs evaluated
template <class Query, int W, class Finish>
int64_t host_tile_walk(const std::vector<Query>& queries, const HostTiles& m, LaneOrder order, Finish finish) {
    constexpr int kScan = W == 1 ? 1 : Query::kScan;
    const float inf = bits_float(kMdInfBits);
    int64_t evaluated = 0;
    for (size_t i0 = 0; i0 < queries.size(); i0 += W) {
        const Query* q = queries.data() + i0;
        const int lanes = queries.size() - i0 < W ? (int)(queries.size() - i0) : W;
        TileWinner won[W];
        int64_t nearest[W];
        const auto evaluate = [&](int64_t t) {
            host_tile_eval(q, lanes, m, t, won);
            evaluated += 1;
        };
        for (int l = 0; l < lanes; ++l) {
            won[l] = TileWinner{inf, -1}, nearest[l] = -1;
            float least = inf, value;
            for (int64_t t = 0; t < m.tiles; ++t)
                if (q[l].rank(m.boxes[t], &value) && value < least) least = value, nearest[l] = t;
        }
        for (int l = 0; l < lanes; ++l) {          // the nearest tiles, each once: that of the lowest lane that still waits goes first
            bool before = nearest[l] < 0;
            for (int k = 0; k < l; ++k) before = before || nearest[k] == nearest[l];
            if (!before) evaluate(nearest[l]);
        }
        for (int64_t s0 = 0; s0 < m.tiles; s0 += kScan) {
            typename Query::Memo memo[kScan][W];
            const int n = m.tiles - s0 < kScan ? (int)(m.tiles - s0) : kScan;
            for (int k = 0; k < n; ++k)
                for (int l = 0; l < lanes; ++l) memo[k][l] = q[l].recall(m.boxes[order(s0 + k, m.tiles)], won[l].best);
            for (int k = 0; k < n; ++k) {
                const int64_t t = order(s0 + k, m.tiles);
                bool needed = false, before = false;
                for (int l = 0; l < lanes; ++l) needed = needed || q[l].needs(memo[k][l], won[l].best), before = before || nearest[l] == t;
                if (needed && !before) evaluate(t);
            }
        }
        for (int l = 0; l < lanes; ++l) finish(i0 + l, won[l].best, won[l].face);
    }
    return evaluated;
}

// tile_sweep<Query, true> (tile_walk.h) the same way; finish(i, state) stores what the kernel stores for query i.  A lane's need of a
// tile does not depend on what it has found, so the scan groups leave no trace and a wave of one lane evaluates what the lane reaches
template <class Query, int W, class Finish>
int64_t host_tile_sweep(const std::vector<Query>& queries, const HostTiles& m, LaneOrder order, Finish finish) {
    int64_t evaluated = 0;
    for (size_t i0 = 0; i0 < queries.size(); i0 += W) {
        const Query* q = queries.data() + i0;
        const int lanes = queries.size() - i0 < W ? (int)(queries.size() - i0) : W;
        typename Query::State state[W] = {};
        for (int64_t s = 0; s < m.tiles; ++s) {
            const int64_t t = order(s, m.tiles);
            bool needed = false;
            for (int l = 0; l < lanes; ++l) needed = needed || q[l].reaches(m.boxes[t]);
            if (!needed) continue;
            host_tile_eval(q, lanes, m, t, state);
            evaluated += 1;
        }
        for (int l = 0; l < lanes; ++l) finish(i0 + l, state[l]);
    }
    return evaluated;
}

// the tail of an output file: int64 violations, evaluated, pairs.  -> the program's exit status
inline int write_tail(FILE* fo, bool ok, int64_t violations, int64_t evaluated, int64_t pairs) {
    const int64_t tail[3] = {violations, evaluated, pairs};
    ok = ok && std::fwrite(tail, 8, 3, fo) == 3;
    return std::fclose(fo) == 0 && ok ? 0 : 2;
}

}  // namespace npcd
