// The k-d tree of the keyframe's depth association (KeyFrame.cpp:1151-1158), restated exactly from the reference's
// src/utils/KDTree.hpp so that every query gets the reference's nearest point, ties included:
//   build    (:187-205)  split [lo, hi) at mid = (n - 1) / 2 with std::nth_element on axis depth % 2, recurse on both sides;
//   distance (:253-259)  sqrt(0 + dx*dx + dy*dy), every product and sum rounded on its own (the reference has no FMA: C++14, no -march);
//   nnSearch (:99-112, :263-284)  visit the node, replace the guess only on a strict `<`, descend the near side first
//                        (dir = query[axis] < train[axis] ? 0 : 1), then the far side when fabs(query[axis] - train[axis]) < minDist.
// So the first point of that traversal at the smallest sqrt distance wins an exact tie — not the lowest index.  The tree's shape, hence
// a tie's winner, depends on std::nth_element's permutation, which the standard leaves to the library: it is pinned for libstdc++
// (tests/test_kdtree_pin.py against the reference's own tree, tests/golden/kdtree/ref_kdtree_*.npz).
//
// Layout: after the recursive in-place partition the index array IS the tree — node [lo, hi) is perm[lo + (hi - lo - 1) / 2], its
// children are [lo, mid) and [mid + 1, hi).  The caller gathers the coordinates (and whatever rides with them) in that order; the walk
// returns a position in it.  Plain C++ outside hipcc (tests/host_logic/harness.cpp compiles it with g++).
#pragma once
#include <math.h>

#include <algorithm>
#include <numeric>

#if defined(__HIPCC__)
#define EDS_KD_HD __host__ __device__ inline
#else
#define EDS_KD_HD inline
#endif

namespace edskd {

constexpr int STACK = 32;        // depth <= ceil(log2(m + 1)) <= 31 for every int m: at most one pending far side per level

// host: perm[0, n) holds point indices on entry (0..m-1 at the root); partitions it in place into the tree (KDTree.hpp:187-205)
inline void build(const double* xy, int* perm, int n, int depth = 0) {
    while (n > 0) {
        const int axis = depth % 2, mid = (n - 1) / 2;
        std::nth_element(perm, perm + mid, perm + n, [&](int lhs, int rhs) { return xy[2 * (size_t)lhs + axis] < xy[2 * (size_t)rhs + axis]; });
        build(xy, perm, mid, depth + 1);
        perm += mid + 1; n -= mid + 1; ++depth;          // the right side: the recursion's tail call
    }
}
inline void build_tree(const double* xy, int m, int* perm) {
    std::iota(perm, perm + m, 0);
    build(xy, perm, m, 0);
}

// nnSearch over txy (m x 2, the tree's order): returns the winner's position in that order and its minDist
EDS_KD_HD int nn(const double* txy, int m, double qx, double qy, double* min_dist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int lo_s[STACK], hi_s[STACK], dep_s[STACK];
    double diff_s[STACK];
    int sp = 0, guess = 0;
    double best = 1.79769313486231570815e+308;           // std::numeric_limits<double>::max()
    int lo = 0, hi = m, depth = 0;
    for (;;) {
        if (lo < hi) {
            const int mid = lo + (hi - lo - 1) / 2, axis = depth & 1;
            const double tx = txy[2 * (size_t)mid], ty = txy[2 * (size_t)mid + 1];
            const double dx = qx - tx, dy = qy - ty;
            double d2 = 0;
            d2 += dx * dx;
            d2 += dy * dy;
            const double dist = sqrt(d2);
            if (dist < best) { best = dist; guess = mid; }
            const double q = axis ? qy : qx, t = axis ? ty : tx;
            const bool dir = !(q < t);
            // the far side waits; its prune test is made when it is popped, against the minDist of that moment (:281-283)
            lo_s[sp] = dir ? lo : mid + 1; hi_s[sp] = dir ? mid : hi; dep_s[sp] = depth + 1; diff_s[sp] = fabs(q - t); ++sp;
            if (dir) lo = mid + 1; else hi = mid;
            ++depth;
            continue;
        }
        do {
            if (sp == 0) { if (min_dist) *min_dist = best; return guess; }
            --sp;
        } while (!(diff_s[sp] < best));
        lo = lo_s[sp]; hi = hi_s[sp]; depth = dep_s[sp];
    }
}

}  // namespace edskd
