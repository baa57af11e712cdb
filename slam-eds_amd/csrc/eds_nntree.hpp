// The k-d tree of CoarseInitializer::makeNN (CoarseInitializer.cpp:884-958), restated from the reference's src/utils/nanoflann.h
// (quoted as N:n) so that every point gets nanoflann's ten neighbours and nanoflann's parent IN NANOFLANN'S ORDER, ties included.  The
// reference instantiates KDTreeSingleIndexAdaptor<L2_Simple_Adaptor<float, FLANNPointcloud>, FLANNPointcloud, 2> with leaf size 5 and
// asks it through KNNResultSet<float, int, int>(10) and (1) with SearchParams() (eps = 0).  What decides a tie, and is restated:
//   build  N:985-991 vind = 0 .. n-1;  N:1024-1046 the root box from the points;  N:1056-1104 divideTree — a node of <= 5 points is a
//          leaf with the box of its points, otherwise middleSplit_, the children under copies of the box cut at cutval, divlow / divhigh
//          from the children's boxes after they were tightened, and the node's box the union of the two;  N:1118-1157 middleSplit_ —
//          the dimension (with N:1134's spread taken along the current cutfeat, so dimension 1 is chosen only where dimension 0's span
//          fails `span > (1 - EPS) max_span`), split_val = (low + high) / 2 clamped to the points' range, index = lim1 if lim1 >
//          count/2, lim2 if lim2 < count/2, else count/2;  N:1169-1196 planeSplit's two swap passes;
//   walk   N:1198-1215 the query's squared distance to the root box per dimension;  N:1222-1269 searchLevel — a leaf tests
//          dist < worst_dist against the worst distance as it was ON ENTRY to the leaf, an inner node descends child1 first when
//          diff1 + diff2 < 0 and the other child afterwards when (mindistsq + cut_dist) - dists[idx] <= worstDist();
//   set    N:104-145 KNNResultSet: the last distance starts at FLT_MAX, addPoint (without NANOFLANN_FIRST_MATCH) puts a new point
//          BEHIND the held points of equal distance and drops what falls off the end.
// The distance is FLANNPointcloud::kdtree_distance: d0 d0 + d1 d1 of the fp32 u, v, every operation rounded on its own (the reference
// has no FMA: C++14, no -march) — the walk is compiled with contraction off.  Pinned by tests/test_nn_pin.py against the reference's
// own nanoflann (tests/golden/nn/ref_nn_*.npz) and a numpy restatement (tests/np_nn_oracle.py).
//
// Layout: nodes in the order divideTree allocates them, so child1 of node k is node k + 1 and only child2 is stored; a leaf has
// child2 < 0 and [left, right) into vind.  knn() walks with an explicit stack of the pending `other` children — one per level at most,
// each with the mindistsq and the per-dimension distances it would be entered with (searchLevel restores dists[idx] on the way up, so
// these are values known when the node is left for its first child; only the prune test waits for the pop, against the worst distance
// of that moment).  A tree deeper than STACK is walked by knn_recursive on the host.  Plain C++ outside hipcc.
//
// Coordinates are finite (the C entry points refuse others).  For anything else the build still ends: a split that would leave a side
// empty — which finite coordinates cannot produce — is moved to count/2.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define EDS_NN_HD __host__ __device__ inline
#else
#define EDS_NN_HD inline
#endif

namespace edsnn {

constexpr int LEAF = 5;          // KDTreeSingleIndexAdaptorParams(5)
constexpr int STACK = 64;        // pending far sides of the explicit walk: one per level of the tree
constexpr float FLT_MAX_ = 3.40282346638528859812e+38f;

struct Node {
    int32_t child2;              // < 0: a leaf
    int32_t feat;                // divfeat
    int32_t left, right;         // a leaf's [left, right) into vind
    float divlow, divhigh;
};
struct Box { float low[2], high[2]; };

struct Tree {
    std::vector<Node> nodes;     // empty for n = 0
    std::vector<int32_t> vind;
    Box box;                     // the root box after the build
    int depth = 0;               // inner nodes above the deepest leaf: what the explicit walk's stack must hold
};

namespace detail {

struct Builder {
    const float* uv;
    Tree& t;
    float get(int32_t idx, int dim) const { return uv[2 * (size_t)idx + dim]; }

    void min_max(const int32_t* ind, int count, int element, float& lo, float& hi) const {
        lo = hi = get(ind[0], element);
        for (int i = 1; i < count; ++i) {
            const float v = get(ind[i], element);
            if (v < lo) lo = v;
            if (v > hi) hi = v;
        }
    }

    // N:1169-1196; left and right are unsigned there, and `right` stops at 0
    void plane_split(int32_t* ind, int count, int cutfeat, float cutval, int& lim1, int& lim2) const {
        int left = 0, right = count - 1;
        for (;;) {
            while (left <= right && get(ind[left], cutfeat) < cutval) ++left;
            while (right && left <= right && get(ind[right], cutfeat) >= cutval) --right;
            if (left > right || !right) break;
            const int32_t s = ind[left]; ind[left] = ind[right]; ind[right] = s;
            ++left; --right;
        }
        lim1 = left;
        right = count - 1;
        for (;;) {
            while (left <= right && get(ind[left], cutfeat) <= cutval) ++left;
            while (right && left <= right && get(ind[right], cutfeat) > cutval) --right;
            if (left > right || !right) break;
            const int32_t s = ind[left]; ind[left] = ind[right]; ind[right] = s;
            ++left; --right;
        }
        lim2 = left;
    }

    // N:1118-1157
    void middle_split(int32_t* ind, int count, int& index, int& cutfeat, float& cutval, const Box& b) const {
        const float EPS = 0.00001f;
        float max_span = b.high[0] - b.low[0];
        { const float span = b.high[1] - b.low[1]; if (span > max_span) max_span = span; }
        float max_spread = -1.0f;
        cutfeat = 0;
        for (int i = 0; i < 2; ++i) {
            const float span = b.high[i] - b.low[i];
            if (span > (1 - EPS) * max_span) {
                float lo, hi;
                min_max(ind, count, cutfeat, lo, hi);         // N:1134: along cutfeat, not along i
                const float spread = hi - lo;
                if (spread > max_spread) { cutfeat = i; max_spread = spread; }
            }
        }
        const float split_val = (b.low[cutfeat] + b.high[cutfeat]) / 2;
        float lo, hi;
        min_max(ind, count, cutfeat, lo, hi);
        if (split_val < lo) cutval = lo;
        else if (split_val > hi) cutval = hi;
        else cutval = split_val;
        int lim1, lim2;
        plane_split(ind, count, cutfeat, cutval, lim1, lim2);
        if (lim1 > count / 2) index = lim1;
        else if (lim2 < count / 2) index = lim2;
        else index = count / 2;
        if (index < 1 || index >= count) index = count / 2;   // not with finite coordinates: see the head of the file
    }

    // N:1056-1104; returns the node's position
    int32_t divide(int left, int right, Box& b, int depth) {
        if (depth > t.depth) t.depth = depth;
        const int32_t me = (int32_t)t.nodes.size();
        t.nodes.push_back(Node{-1, 0, left, right, 0.0f, 0.0f});
        int32_t* vind = t.vind.data();
        if (right - left <= LEAF) {
            for (int i = 0; i < 2; ++i) b.low[i] = b.high[i] = get(vind[left], i);
            for (int k = left + 1; k < right; ++k)
                for (int i = 0; i < 2; ++i) {
                    const float v = get(vind[k], i);
                    if (b.low[i] > v) b.low[i] = v;
                    if (b.high[i] < v) b.high[i] = v;
                }
            return me;
        }
        int idx, cutfeat;
        float cutval;
        middle_split(vind + left, right - left, idx, cutfeat, cutval, b);
        Box lb = b;
        lb.high[cutfeat] = cutval;
        divide(left, left + idx, lb, depth + 1);
        Box rb = b;
        rb.low[cutfeat] = cutval;
        const int32_t c2 = divide(left + idx, right, rb, depth + 1);
        Node& nd = t.nodes[me];
        nd.child2 = c2;
        nd.feat = cutfeat;
        nd.left = nd.right = 0;
        nd.divlow = lb.high[cutfeat];
        nd.divhigh = rb.low[cutfeat];
        for (int i = 0; i < 2; ++i) {
            b.low[i] = lb.low[i] < rb.low[i] ? lb.low[i] : rb.low[i];
            b.high[i] = lb.high[i] > rb.high[i] ? lb.high[i] : rb.high[i];
        }
        return me;
    }
};

}  // namespace detail

// host: buildIndex() over uv (n x {u, v})
inline void build(const float* uv, int n, Tree& t) {
    t.nodes.clear();
    t.vind.resize(n > 0 ? n : 0);
    t.depth = 0;
    t.box = Box{{0.0f, 0.0f}, {0.0f, 0.0f}};
    if (n <= 0) return;
    for (int i = 0; i < n; ++i) t.vind[i] = i;
    t.nodes.reserve(2 * (size_t)n);
    detail::Builder b{uv, t};
    for (int i = 0; i < 2; ++i) t.box.low[i] = t.box.high[i] = b.get(0, i);
    for (int k = 1; k < n; ++k)
        for (int i = 0; i < 2; ++i) {
            if (b.get(k, i) < t.box.low[i]) t.box.low[i] = b.get(k, i);
            if (b.get(k, i) > t.box.high[i]) t.box.high[i] = b.get(k, i);
        }
    b.divide(0, n, t.box, 0);
}

// KNNResultSet<float, int, int>(K) over idx / dist (N:92-151)
template <int K>
struct ResultSet {
    int32_t* idx;
    float* dist;
    int count;
    EDS_NN_HD ResultSet(int32_t* i, float* d) : idx(i), dist(d), count(0) { dist[K - 1] = FLT_MAX_; }
    EDS_NN_HD float worst() const { return dist[K - 1]; }
    EDS_NN_HD void add(float d, int32_t index) {
        int i;
        for (i = count; i > 0; --i) {
            if (dist[i - 1] > d) {
                if (i < K) { dist[i] = dist[i - 1]; idx[i] = idx[i - 1]; }
            } else break;
        }
        if (i < K) { dist[i] = d; idx[i] = index; }
        if (count < K) count++;
    }
};

// one leaf of searchLevel (N:1226-1237)
template <int K>
EDS_NN_HD void scan_leaf(const Node& nd, const int32_t* vind, const float* uv, float q0, float q1, ResultSet<K>& rs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float worst = rs.worst();
    for (int i = nd.left; i < nd.right; ++i) {
        const int32_t j = vind[i];
        const float d0 = q0 - uv[2 * (size_t)j], d1 = q1 - uv[2 * (size_t)j + 1];
        const float d = d0 * d0 + d1 * d1;
        if (d < worst) rs.add(d, j);
    }
}

// computeInitialDistances (N:1198-1215)
EDS_NN_HD float initial_distances(const Box& b, const float* q, float* dists) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float distsq = 0.0f;
    for (int i = 0; i < 2; ++i) {
        dists[i] = 0.0f;
        if (q[i] < b.low[i]) { dists[i] = (q[i] - b.low[i]) * (q[i] - b.low[i]); distsq += dists[i]; }
        if (q[i] > b.high[i]) { dists[i] = (q[i] - b.high[i]) * (q[i] - b.high[i]); distsq += dists[i]; }
    }
    return distsq;
}

// findNeighbors with a KNNResultSet(K) for a tree of depth <= STACK (n_nodes > 0).  idx[K] / dist[K] must hold -1 / 0 on entry: what
// the search never writes stays so (fewer than K points), except that dist[K - 1] is FLT_MAX until the set is full.  Returns the
// number found.
template <int K>
EDS_NN_HD int knn(const Node* nodes, const int32_t* vind, const float* uv, const Box& box, float q0, float q1, int32_t* idx, float* dist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    ResultSet<K> rs(idx, dist);
    const float q[2] = {q0, q1};
    float dd[2];
    float mind = initial_distances(box, q, dd);
    int32_t node_s[STACK];
    float mind_s[STACK], d0_s[STACK], d1_s[STACK];
    int sp = 0;
    int32_t node = 0;
    for (;;) {
        const Node nd = nodes[node];
        if (nd.child2 < 0) {
            scan_leaf<K>(nd, vind, uv, q0, q1, rs);
            do {
                if (sp == 0) return rs.count;
                --sp;
            } while (!(mind_s[sp] <= rs.worst()));
            node = node_s[sp]; mind = mind_s[sp]; dd[0] = d0_s[sp]; dd[1] = d1_s[sp];
            continue;
        }
        const float val = nd.feat ? q1 : q0;
        const float diff1 = val - nd.divlow, diff2 = val - nd.divhigh;
        const bool low_first = (diff1 + diff2) < 0;
        const float cut = low_first ? (val - nd.divhigh) * (val - nd.divhigh) : (val - nd.divlow) * (val - nd.divlow);
        const float dst = nd.feat ? dd[1] : dd[0];
        if (sp == STACK) return -1;                           // a tree deeper than the stack: the caller measured the depth, so never
        node_s[sp] = low_first ? nd.child2 : node + 1;
        mind_s[sp] = mind + cut - dst;
        d0_s[sp] = nd.feat ? dd[0] : cut;
        d1_s[sp] = nd.feat ? cut : dd[1];
        ++sp;
        node = low_first ? node + 1 : nd.child2;
    }
}

// searchLevel as the reference writes it, by recursion: for trees deeper than STACK
template <int K>
inline void search_level(const Tree& t, const float* uv, ResultSet<K>& rs, const float* q, int32_t node, float mindistsq, float* dists) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Node& nd = t.nodes[node];
    if (nd.child2 < 0) { scan_leaf<K>(nd, t.vind.data(), uv, q[0], q[1], rs); return; }
    const int idx = nd.feat;
    const float val = q[idx];
    const float diff1 = val - nd.divlow, diff2 = val - nd.divhigh;
    int32_t best, other;
    float cut;
    if ((diff1 + diff2) < 0) { best = node + 1; other = nd.child2; cut = (val - nd.divhigh) * (val - nd.divhigh); }
    else { best = nd.child2; other = node + 1; cut = (val - nd.divlow) * (val - nd.divlow); }
    search_level<K>(t, uv, rs, q, best, mindistsq, dists);
    const float dst = dists[idx];
    mindistsq = mindistsq + cut - dst;
    dists[idx] = cut;
    if (mindistsq <= rs.worst()) search_level<K>(t, uv, rs, q, other, mindistsq, dists);
    dists[idx] = dst;
}
template <int K>
inline int knn_recursive(const Tree& t, const float* uv, float q0, float q1, int32_t* idx, float* dist) {
    ResultSet<K> rs(idx, dist);
    const float q[2] = {q0, q1};
    float dd[2];
    const float mind = initial_distances(t.box, q, dd);
    search_level<K>(t, uv, rs, q, 0, mind, dd);
    return rs.count;
}

// host: a query against a built tree — the explicit walk where the tree fits `stack` (<= STACK), the recursion otherwise
template <int K>
inline int knn_host(const Tree& t, const float* uv, float q0, float q1, int32_t* idx, float* dist, int stack = STACK) {
    for (int k = 0; k < K; ++k) { idx[k] = -1; dist[k] = 0.0f; }
    if (t.nodes.empty()) return 0;
    const int found = t.depth <= (stack < STACK ? stack : STACK) ? knn<K>(t.nodes.data(), t.vind.data(), uv, t.box, q0, q1, idx, dist)
                                                                 : knn_recursive<K>(t, uv, q0, q1, idx, dist);
    for (int k = found < 0 ? 0 : found; k < K; ++k) dist[k] = 0.0f;
    return found;
}

}  // namespace edsnn
