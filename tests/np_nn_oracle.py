"""CoarseInitializer::makeNN (CoarseInitializer.cpp:884-958) restated in plain Python from reading the reference's nanoflann
(src/utils/nanoflann.h, quoted as N:n) — test oracle, independent of the product's C++.  Every fp32 value is an np.float32 scalar, so
each difference, product and sum rounds on its own, as the reference's build (C++14, no -march: no FMA) rounds it.

    tree = build(uv)                 KDTreeSingleIndexAdaptor<L2_Simple_Adaptor<float, PC>, PC, 2>(…, Params(5)).buildIndex()
    knn(tree, q, k)                  KNNResultSet<float, int, int>(k).init(…); findNeighbors(…, SearchParams())
    make_nn(uv, uv_up)               the two searches of :915-946 for every point

What is restated, and where a tie's winner comes from:
  * N:985-991 vind = 0 .. n-1; N:1024-1046 the root box from the points (kdtree_get_bbox returns false);
  * N:1056-1104 divideTree: a node of <= 5 points is a leaf with the box of its points; otherwise middleSplit_, the left child under a
    copy of the box cut at high = cutval, the right under one cut at low = cutval, divlow = the left child's (now tight) high, divhigh =
    the right child's low, and the node's box becomes the union of its children's;
  * N:1118-1157 middleSplit_: cutfeat is the first dimension whose span exceeds (1 - EPS) max_span and whose spread is larger than the
    best so far — where the spread is measured along the CURRENT cutfeat (N:1134 passes cutfeat, not i), so dimension 1 is chosen only
    when dimension 0's span fails the test; split_val = (low + high) / 2 clamped to the points' range; index = lim1 if lim1 > count/2,
    lim2 if lim2 < count/2, else count/2;
  * N:1169-1196 planeSplit: the two swap passes, with their unsigned `right` that stops at 0;
  * N:1198-1215 the query's distance to the root box per dimension; N:1222-1269 searchLevel: a leaf tests dist < worst_dist against
    the worst distance AS IT WAS ON ENTRY to the leaf; an inner node takes child1 first when diff1 + diff2 < 0, then the other child
    when mindistsq + cut_dist - dists[idx] <= worstDist() (epsError = 1);
  * N:124-145 KNNResultSet::addPoint without NANOFLANN_FIRST_MATCH: a new point goes BEHIND the held points of equal distance.
"""
import sys

import numpy as np

F = np.float32
NN = 10
LEAF = 5
FLT_MAX = np.finfo(np.float32).max
EPS = F(0.00001)


class Tree:
    """uv (n x 2 fp32), vind (the permuted indices), root (nested node tuples), box (the root box after the build), depth (levels of
    inner nodes above the deepest leaf)"""


def _divide(t, left, right, box, depth):
    """N:1056-1104.  box = [[low0, high0], [low1, high1]], changed in place as the reference changes its reference argument."""
    t.depth = max(t.depth, depth)
    uv, vind = t.uv, t.vind
    if right - left <= LEAF:
        for i in range(2):
            box[i][0] = box[i][1] = uv[vind[left], i]
        for k in range(left + 1, right):
            for i in range(2):
                v = uv[vind[k], i]
                if box[i][0] > v: box[i][0] = v
                if box[i][1] < v: box[i][1] = v
        return ("leaf", left, right)
    idx, cutfeat, cutval = _middle_split(t, left, right - left, box)
    lbox = [list(box[0]), list(box[1])]
    lbox[cutfeat][1] = cutval
    c1 = _divide(t, left, left + idx, lbox, depth + 1)
    rbox = [list(box[0]), list(box[1])]
    rbox[cutfeat][0] = cutval
    c2 = _divide(t, left + idx, right, rbox, depth + 1)
    divlow, divhigh = lbox[cutfeat][1], rbox[cutfeat][0]
    for i in range(2):
        box[i][0] = min(lbox[i][0], rbox[i][0])
        box[i][1] = max(lbox[i][1], rbox[i][1])
    return ("node", cutfeat, divlow, divhigh, c1, c2)


def _min_max(t, off, count, element):
    vals = [t.uv[t.vind[off + i], element] for i in range(count)]
    lo = hi = vals[0]
    for v in vals[1:]:
        if v < lo: lo = v
        if v > hi: hi = v
    return lo, hi


def _middle_split(t, off, count, box):
    """N:1118-1157"""
    max_span = box[0][1] - box[0][0]
    span = box[1][1] - box[1][0]
    if span > max_span:
        max_span = span
    max_spread = F(-1)
    cutfeat = 0
    for i in range(2):
        span = box[i][1] - box[i][0]
        if span > (F(1) - EPS) * max_span:
            lo, hi = _min_max(t, off, count, cutfeat)           # N:1134: along cutfeat, not along i
            spread = hi - lo
            if spread > max_spread:
                cutfeat = i
                max_spread = spread
    split_val = (box[cutfeat][0] + box[cutfeat][1]) / F(2)
    lo, hi = _min_max(t, off, count, cutfeat)
    cutval = lo if split_val < lo else hi if split_val > hi else split_val
    lim1, lim2 = _plane_split(t, off, count, cutfeat, cutval)
    half = count // 2
    index = lim1 if lim1 > half else lim2 if lim2 < half else half
    return index, cutfeat, cutval


def _plane_split(t, off, count, cutfeat, cutval):
    """N:1169-1196; left and right are unsigned there: `right` never passes below 0"""
    uv, ind = t.uv, t.vind

    def get(k):
        return uv[ind[off + k], cutfeat]

    def swap(a, b):
        ind[off + a], ind[off + b] = ind[off + b], ind[off + a]

    left, right = 0, count - 1
    while True:
        while left <= right and get(left) < cutval: left += 1
        while right and left <= right and get(right) >= cutval: right -= 1
        if left > right or not right: break
        swap(left, right)
        left += 1
        right -= 1
    lim1 = left
    right = count - 1
    while True:
        while left <= right and get(left) <= cutval: left += 1
        while right and left <= right and get(right) > cutval: right -= 1
        if left > right or not right: break
        swap(left, right)
        left += 1
        right -= 1
    return lim1, left


def build(uv):
    t = Tree()
    t.uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    n = len(t.uv)
    t.vind = list(range(n))
    t.root, t.box, t.depth = None, None, 0
    if n == 0:
        return t
    box = [[t.uv[0, 0], t.uv[0, 0]], [t.uv[0, 1], t.uv[0, 1]]]
    for k in range(1, n):
        for i in range(2):
            v = t.uv[k, i]
            if v < box[i][0]: box[i][0] = v
            if v > box[i][1]: box[i][1] = v
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 1000))
    t.root = _divide(t, 0, n, box, 0)
    t.box = box
    return t


class _ResultSet:
    """N:92-151"""

    def __init__(self, capacity):
        self.capacity, self.count = capacity, 0
        self.indices, self.dists = [-1] * capacity, [F(0)] * capacity
        self.dists[capacity - 1] = FLT_MAX

    def add(self, dist, index):
        i = self.count
        while i > 0:
            if self.dists[i - 1] > dist:
                if i < self.capacity:
                    self.dists[i], self.indices[i] = self.dists[i - 1], self.indices[i - 1]
            else:
                break
            i -= 1
        if i < self.capacity:
            self.dists[i], self.indices[i] = dist, index
        if self.count < self.capacity:
            self.count += 1

    def worst(self):
        return self.dists[self.capacity - 1]


def _search(t, rs, q, node, mindistsq, dists):
    """N:1222-1269"""
    if node[0] == "leaf":
        worst = rs.worst()
        for i in range(node[1], node[2]):
            j = t.vind[i]
            d0 = q[0] - t.uv[j, 0]
            d1 = q[1] - t.uv[j, 1]
            dist = d0 * d0 + d1 * d1
            if dist < worst:
                rs.add(dist, j)
        return
    _, idx, divlow, divhigh, c1, c2 = node
    val = q[idx]
    diff1, diff2 = val - divlow, val - divhigh
    if diff1 + diff2 < 0:
        best, other, cut = c1, c2, (val - divhigh) * (val - divhigh)
    else:
        best, other, cut = c2, c1, (val - divlow) * (val - divlow)
    _search(t, rs, q, best, mindistsq, dists)
    dst = dists[idx]
    mindistsq = mindistsq + cut - dst
    dists[idx] = cut
    if mindistsq <= rs.worst():
        _search(t, rs, q, other, mindistsq, dists)
    dists[idx] = dst


def knn(t, q, k):
    """(indices, squared distances) as findNeighbors leaves them in arrays that held -1 and 0: the places it never wrote stay so"""
    rs = _ResultSet(k)
    if t.root is not None:
        q = (F(q[0]), F(q[1]))
        dists = [F(0), F(0)]
        distsq = F(0)
        for i in range(2):
            if q[i] < t.box[i][0]:
                dists[i] = (q[i] - t.box[i][0]) * (q[i] - t.box[i][0])
                distsq = distsq + dists[i]
            if q[i] > t.box[i][1]:
                dists[i] = (q[i] - t.box[i][1]) * (q[i] - t.box[i][1])
                distsq = distsq + dists[i]
        _search(t, rs, q, t.root, distsq, dists)
    idx = np.array(rs.indices, dtype=np.int32)
    return idx, np.where(idx < 0, F(0), np.array(rs.dists, dtype=np.float32))


def make_nn(uv, uv_up=None):
    """dict(nb n x 10, dist n x 10, parent n, parent_dist n, depth, depth_up): -1 / 0 where nanoflann writes nothing"""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    up = np.zeros((0, 2), np.float32) if uv_up is None else np.ascontiguousarray(uv_up, dtype=np.float32).reshape(-1, 2)
    n = len(uv)
    nb, dist = np.full((n, NN), -1, np.int32), np.zeros((n, NN), np.float32)
    parent, parent_dist = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t, tu = build(uv), build(up)
        for i in range(n):
            nb[i], dist[i] = knn(t, uv[i], NN)
            if len(up):
                q = (uv[i, 0] * F(0.5) - F(0.25), uv[i, 1] * F(0.5) - F(0.25))
                pi, pd = knn(tu, q, 1)
                parent[i], parent_dist[i] = pi[0], pd[0]
    return dict(nb=nb, dist=dist, parent=parent, parent_dist=parent_dist, depth=t.depth, depth_up=tu.depth)


def exhaustive(uv):
    """the rule the product had before the pin — the ten smallest fp32 squared distances, ties to the lower index — for the tests that
    show the goldens tell the two apart"""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    d0 = uv[:, None, 0] - uv[None, :, 0]
    d1 = uv[:, None, 1] - uv[None, :, 1]
    d = d0 * d0 + d1 * d1                                      # numpy rounds every product and sum on its own
    order = np.argsort(d, axis=1, kind="stable")[:, :NN].astype(np.int32)
    out = np.full((len(uv), NN), -1, np.int32)
    out[:, :order.shape[1]] = order
    return out
