// Connected components of the inside nodes of a lattice: the union-find and the three phases of csrc/components.hip,
// written once for the device and the host.  The kernels run them with integer atomics on LDS and global memory, the stand-alone
// program csrc/components_host.cpp runs the same functions as plain loops over workgroups and lanes (tests/test_components_cpu.py):
// this header includes nothing of HIP.
//
//   Inside: f > level (NaN: outside), the isosurface's test.  Adjacent: the two ends of one of the seven edge types (csrc/isosurface.hip),
//   14 neighbours a node.  Label: the smallest node index (z gy + y) gx + x of the component; -1 outside.
//
// The forest.  parent[i] is -1 for an outside node and otherwise the index of an inside node of i's component with
//   (I)  parent[i] <= i,
// a root being its own parent.  An entry changes only by an integer minimum with the index of a node of the same component that is
// smaller than the entry's own index: (I) holds throughout, an entry never rises, and every value an entry has ever held is a node
// of its component.  So a reader that sees an older value of an entry -- another workgroup's minimum not yet visible to it --
// still walks inside the component and still downward.
//
// Loop bounds, none of which waits for another lane's progress:
//   cc_root / cc_find   follow i -> parent[i] while parent[i] != i; by (I) the index falls strictly: at most i steps.
//   cc_union(a, b)      takes the two roots, a > b, and lowers parent[a] to b.  If the minimum returns a, the root a has been linked:
//                       done.  Otherwise another lane had linked a below `old` < a in the meantime; whether or not the minimum
//                       replaced that link by a -> b, a stays joined to b or to old, and joining old with b finishes the job.  The larger
//                       of the pair was a and is now max(root(old), root(b)) <= max(old, b) < a: it falls strictly with every retry,
//                       so the retries are bounded by the index a lane started with -- a label can only decrease so often.
// Whether an entry is negative never changes, so "inside" is read with a plain load at any time.
// Minimum and (for the sizes) addition of integers commute: the labels and sizes are the same bits whatever the schedule.
#pragma once
#include <stdint.h>

#include "bits.h"          // NPCD_HD

namespace npcd {

// the brick of nodes one workgroup labels in LDS (x fastest), and how its lanes share it
constexpr int kCcBrickX = 16, kCcBrickY = 8, kCcBrickZ = 8;
constexpr int kCcBrickNodes = kCcBrickX * kCcBrickY * kCcBrickZ;          // 1,024 labels and 1,024 counts = 8 KB of LDS
constexpr int kCcThreads = 256;
constexpr int kCcNodesPerLane = kCcBrickNodes / kCcThreads;

struct CcGrid {
    int gx, gy, gz, n;                  // nodes per axis and per volume
    int bricks_x, bricks_y, bricks;          // bricks per row, per slab of bricks, per volume
};
NPCD_HD CcGrid cc_grid(int gz, int gy, int gx) {
    CcGrid g;
    g.gx = gx, g.gy = gy, g.gz = gz, g.n = gz * gy * gx;
    g.bricks_x = (gx + kCcBrickX - 1) / kCcBrickX;
    g.bricks_y = (gy + kCcBrickY - 1) / kCcBrickY;
    g.bricks = g.bricks_x * g.bricks_y * ((gz + kCcBrickZ - 1) / kCcBrickZ);
    return g;
}

// node l of a brick: local (lx, ly, lz) = (l & 15, l >> 4 & 7, l >> 7), its place in the volume and whether the volume has it.  The
// local order and the volume's order agree inside a brick: both ascend in (z, y, x).
struct CcNode {
    int lx, ly, lz, x, y, z, node;
    bool valid;
};
NPCD_HD CcNode cc_node(const CcGrid& g, int brick, int l) {
    CcNode p;
    const int by = brick / g.bricks_x, bx = brick - by * g.bricks_x, bz = by / g.bricks_y;
    p.lx = l % kCcBrickX, p.ly = l / kCcBrickX % kCcBrickY, p.lz = l / (kCcBrickX * kCcBrickY);
    p.x = bx * kCcBrickX + p.lx, p.y = (by - bz * g.bricks_y) * kCcBrickY + p.ly, p.z = bz * kCcBrickZ + p.lz;
    p.valid = p.x < g.gx && p.y < g.gy && p.z < g.gz;
    p.node = (p.z * g.gy + p.y) * g.gx + p.x;
    return p;
}

// plain memory operations: the host's, and the device's where a launch has no concurrent writer
struct CcPlain {
    static NPCD_HD int load(const int32_t* p) { return *p; }
    static NPCD_HD int fetch_min(int32_t* p, int v) {
        const int old = *p;
        if (v < old) *p = v;
        return old;
    }
    static NPCD_HD void add(int32_t* p, int v) { *p += v; }
};

template <class Ops>
NPCD_HD int cc_root(const int32_t* parent, int i) {
    for (;;) {          // (I): the index falls strictly
        const int p = Ops::load(parent + i);
        if (p == i) return i;
        i = p;
    }
}
// the root, halving the path on the way: an entry is lowered to its grandparent, a node of the component below it
template <class Ops>
NPCD_HD int cc_find(int32_t* parent, int i) {
    for (;;) {
        const int p = Ops::load(parent + i);
        if (p == i) return i;
        const int g = Ops::load(parent + p);
        if (g != p) Ops::fetch_min(parent + i, g);
        i = p;
    }
}
template <class Ops>
NPCD_HD void cc_union(int32_t* parent, int a, int b) {
    for (;;) {          // max(a, b) falls strictly with every retry
        a = cc_find<Ops>(parent, a), b = cc_find<Ops>(parent, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = Ops::fetch_min(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// ---- tile phase: union-find over the edges inside a brick, on the brick's label array `local` [kCcBrickNodes] in local indices, and
// the number of nodes of every piece -- the part of a component inside the brick -- at the piece's root, in `count`
// [kCcBrickNodes].  Four steps with a workgroup barrier between them; every lane runs each step for its kCcNodesPerLane nodes.
NPCD_HD void cc_tile_load(const CcGrid& g, const float* vol, float level, int brick, int l, int32_t* local, int32_t* count) {
    const CcNode p = cc_node(g, brick, l);
    local[l] = p.valid && vol[p.node] > level ? l : -1;
    count[l] = 0;
}
template <class Ops>
NPCD_HD void cc_tile_link(int l, int32_t* local) {
    if (local[l] < 0) return;
    const int lx = l % kCcBrickX, ly = l / kCcBrickX % kCcBrickY, lz = l / (kCcBrickX * kCcBrickY);
    for (int c = 1; c < 8; ++c) {          // the upper end at (dx, dy, dz) = (c & 1, c >> 1 & 1, c >> 2)
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        if (lx + dx >= kCcBrickX || ly + dy >= kCcBrickY || lz + dz >= kCcBrickZ) continue;          // leaves the brick: the merge phase
        const int m = l + dx + dy * kCcBrickX + dz * kCcBrickX * kCcBrickY;
        if (local[m] >= 0) cc_union<Ops>(local, l, m);          // (a node the volume does not have is outside)
    }
}
template <class Ops>
NPCD_HD void cc_tile_count(int l, const int32_t* local, int32_t* count) {          // the forest is complete: plain loads
    if (local[l] >= 0) Ops::add(count + cc_root<CcPlain>(local, l), 1);
}
// the forest of the pieces goes to `parent` in node indices of the volume; sizes = the piece's nodes at its root, 0 elsewhere
NPCD_HD void cc_tile_store(const CcGrid& g, int brick, int l, const int32_t* local, const int32_t* count, int32_t* parent, int32_t* sizes) {
    const CcNode p = cc_node(g, brick, l);
    if (!p.valid) return;
    sizes[p.node] = count[l];
    parent[p.node] = local[l] < 0 ? -1 : cc_node(g, brick, cc_root<CcPlain>(local, l)).node;
}

// ---- merge phase: every edge that leaves a brick joins two trees of the volume's forest `parent` [n].  The walk starts from the
// entries of the two ends as a plain load finds them -- the roots of their pieces, or a node further down: nodes of the same
// components -- and an upper end whose entry equals the one just joined is skipped: the up to four edges from a node into one
// neighbouring brick mostly end in one piece.
template <class Ops>
NPCD_HD void cc_merge_node(const CcGrid& g, int brick, int l, int32_t* parent) {
    const CcNode p = cc_node(g, brick, l);
    if (!p.valid || (p.lx + 1 < kCcBrickX && p.ly + 1 < kCcBrickY && p.lz + 1 < kCcBrickZ)) return;          // no edge leaves the brick
    const int mine = parent[p.node];
    if (mine < 0) return;
    int joined = -1;
    for (int c = 1; c < 8; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        if (p.lx + dx < kCcBrickX && p.ly + dy < kCcBrickY && p.lz + dz < kCcBrickZ) continue;          // inside the brick: done
        if (p.x + dx >= g.gx || p.y + dy >= g.gy || p.z + dz >= g.gz) continue;
        const int other = parent[p.node + dx + dy * g.gx + dz * g.gx * g.gy];
        if (other < 0 || other == joined) continue;
        cc_union<Ops>(parent, mine, other);
        joined = other;
    }
}

// ---- final phase, on a forest that nothing writes any more: the label of a node is its root, and the root of a piece hands the
// piece's nodes on to the component's root -- one integer addition per piece, not per node.  Only a component's root receives
// additions and only a piece's root that is not one clears its own entry: no entry is both.
template <class Ops>
NPCD_HD void cc_final_node(const int32_t* parent, int node, int32_t* labels, int32_t* sizes) {
    const int label = parent[node] < 0 ? -1 : cc_root<CcPlain>(parent, node);
    labels[node] = label;
    if (label < 0 || label == node) return;
    const int piece = sizes[node];
    if (piece > 0) {
        sizes[node] = 0;
        Ops::add(sizes + label, piece);
    }
}

}  // namespace npcd
