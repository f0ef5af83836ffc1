// What the stand-alone host programs (surface_host.cpp, simplify_host.cpp, smooth_host.cpp, mesh_distance_host.cpp,
// components_host.cpp) share: whole-array file I/O, the order in which a loop stands in for the lanes of a launch, and the prefix sums
// that stand in for the kernels' scans.  Host only; not part of libnpcd_hip.so.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

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

}  // namespace npcd
