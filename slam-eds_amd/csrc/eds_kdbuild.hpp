// The depth k-d tree built by SORTING instead of std::nth_element (eds_kdtree.hpp), for the maps where both give the same array.
//
// The node of a sub-range [lo, hi) is its element of rank mid - lo, mid = lo + (hi - lo - 1) / 2, on the level's axis.  If that element's
// axis value occurs once in the sub-range, the node and the SETS on its two sides are unique: they do not depend on how nth_element
// permutes.  Every position of the index array is the median of some sub-range, so by induction the whole array is unique.  A map is
// AMBIGUOUS when at some node the median's axis value equals (==, so -0.0 equals 0.0) that of its predecessor or successor in the node's
// axis-sorted list, or when any coordinate is not finite; an ambiguous map is built by edskd::build_tree and nothing else.
//
// The build keeps two index lists in tree layout, one sorted by x and one by y inside every sub-range.  Level by level (axis = level & 1):
// the node of a sub-range is position mid of the axis' list, the points before it are the left side, those behind it the right side, and
// the OTHER axis' list is partitioned stably by side into [lo, mid) | mid | [mid + 1, hi).  Sub-range bounds follow from m alone
// (segment_of).  After levels(m) levels every position is a node and both lists are the tree.
//
// This header holds what the device kernel (k_kd_build, eds_kdbuild_kernel.hpp) and the host share — the bounds arithmetic, the order of the
// two sorts, the ambiguity rule, the LDS layout — and a serial restatement of the kernel's steps (build_sorted) that the CPU tests compare
// with edskd::build_tree.  Plain C++ outside hipcc.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "eds_kdtree.hpp"

namespace edskdb {

constexpr int CAPACITY = 4096;           // points per map of the device build: what the LDS layout below holds in 160 KiB
constexpr int THREADS = 1024;

// levels after which every position of an m-point tree is a node: the right side of n points has n / 2, so the bit length of m
EDS_KD_HD int levels(int m) {
    int d = 0;
    while (m > 0) { ++d; m >>= 1; }
    return d;
}
EDS_KD_HD int node_of(int lo, int hi) { return lo + (hi - lo - 1) / 2; }

// Position p of an m-point tree at `level`: true with the bounds of the sub-range that still holds it, false (lo = hi = p) when p became
// a node at an earlier level.
EDS_KD_HD bool segment_of(int m, int level, int p, int* lo_out, int* hi_out) {
    int lo = 0, hi = m;
    for (int l = 0; l < level; ++l) {
        const int mid = node_of(lo, hi);
        if (p == mid) { *lo_out = p; *hi_out = p; return false; }
        if (p < mid) hi = mid; else lo = mid + 1;
    }
    *lo_out = lo; *hi_out = hi;
    return true;
}

// the order of both sorts: by axis value, equal values by index (which of two equal values comes first never shows in an unambiguous map)
EDS_KD_HD bool key_before(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// the rule at one node: list = the sub-range's points sorted on `axis`, node at position mid of [lo, hi)
template <class XY, class List>
EDS_KD_HD bool node_ambiguous(const XY& key_of, const List& list, int lo, int hi, int mid) {
    const double k = key_of(list[mid]);
    return (mid > lo && key_of(list[mid - 1]) == k) || (mid + 1 < hi && key_of(list[mid + 1]) == k);
}

EDS_KD_HD bool finite_xy(double x, double y) { return fabs(x) <= 1.79769313486231570815e+308 && fabs(y) <= 1.79769313486231570815e+308; }   // false for NaN

// LDS of k_kd_build for maps of up to M2 points (a power of two): xy (16 M2) | scan (4 M2) | three index lists (3 x 2 M2) | side (M2) | tail
constexpr size_t LDS_TAIL = 256;
EDS_KD_HD int pow2_at_least(int m) {
    int p = 64;                           // at least one wavefront's worth: keeps every part of the layout aligned
    while (p < m) p <<= 1;
    return p;
}
EDS_KD_HD size_t lds_bytes(int M2) { return (size_t)M2 * (16 + 4 + 6 + 1) + LDS_TAIL; }

// Serial restatement of k_kd_build, step for step: returns false when the map is ambiguous (perm is then unspecified), true with
// perm = edskd::build_tree's array otherwise.
inline bool build_sorted(const double* xy, int m, int* perm) {
    for (int i = 0; i < m; ++i) if (!finite_xy(xy[2 * (size_t)i], xy[2 * (size_t)i + 1])) return false;
    std::vector<int> list[3];
    std::vector<unsigned char> side((size_t)m, 0);
    std::vector<uint64_t> scan((size_t)m + 1, 0);     // left count | right count << 32 (the kernel: 16 bits each, m <= CAPACITY)
    for (int a = 0; a < 2; ++a) {
        list[a].resize(m);
        for (int i = 0; i < m; ++i) list[a][i] = i;
        std::sort(list[a].begin(), list[a].end(), [&](int l, int r) { return key_before(xy[2 * (size_t)l + a], l, xy[2 * (size_t)r + a], r); });
    }
    list[2].resize(m);
    int cur[2] = {0, 1}, spare = 2;
    const int D = levels(m);
    for (int level = 0; level < D; ++level) {
        const int a = level & 1;
        const std::vector<int>& A = list[cur[a]];
        const std::vector<int>& O = list[cur[1 - a]];
        std::vector<int>& On = list[spare];
        auto key = [&](int i) { return xy[2 * (size_t)i + a]; };
        bool amb = false;
        for (int p = 0; p < m; ++p) {                     // the sides, and the rule at every node of this level
            int lo, hi;
            if (!segment_of(m, level, p, &lo, &hi)) continue;
            const int mid = node_of(lo, hi);
            side[A[p]] = p < mid ? 0 : (p == mid ? 1 : 2);
            if (p == mid && node_ambiguous(key, A, lo, hi, mid)) amb = true;
        }
        if (amb) return false;
        uint64_t run = 0;
        for (int p = 0; p < m; ++p) {                     // exclusive counts of left (low half) and right (high half) marks in the other list
            scan[p] = run;
            const int s = side[O[p]];
            run += s == 0 ? 1ull : (s == 2 ? 1ull << 32 : 0ull);
        }
        for (int p = 0; p < m; ++p) {                     // stable partition of every sub-range of the other list
            int lo, hi;
            const int i = O[p];
            if (!segment_of(m, level, p, &lo, &hi)) { On[p] = i; continue; }
            const int mid = node_of(lo, hi), s = side[i];
            const uint64_t d = scan[p] - scan[lo];
            On[s == 0 ? lo + (int)(d & 0xffffffffull) : (s == 1 ? mid : mid + 1 + (int)(d >> 32))] = i;
        }
        const int o = cur[1 - a];
        cur[1 - a] = spare; spare = o;
    }
    for (int p = 0; p < m; ++p) perm[p] = list[cur[0]][p];
    return true;
}

}  // namespace edskdb
