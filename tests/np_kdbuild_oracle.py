"""numpy restatement of the sort-based k-d build and its ambiguity rule (slam-eds_amd/csrc/eds_kdbuild.hpp), written recursively and
independently of the product's level-by-level form.

The tree of the depth association (reference src/utils/KDTree.hpp:187-205) splits [lo, hi) at mid = lo + (n - 1) // 2 with
std::nth_element on axis depth % 2.  When the median's axis value occurs once in the sub-range, node and sides are unique as sets, so
sorting gives the same index array.  A map is ambiguous when at some node the median's value equals (==) its predecessor's or successor's
in the node's axis-sorted list, or when a coordinate is not finite."""
import numpy as np


def build_sorted(xy, force=False):
    """(perm, ambiguous).  perm: int64 index array in tree order, None for an ambiguous map unless `force` (then equal values are taken
    in index order, which is NOT what nth_element does: only for showing that the flag matters)."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    m = len(xy)
    if not np.isfinite(xy).all():
        return None, True
    idx = np.arange(m)
    perm = np.full(m, -1, dtype=np.int64)
    rank = np.zeros(m, dtype=np.int64)
    ambiguous = False
    # both lists sorted by value, equal values by index (-0.0 and 0.0 compare equal)
    stack = [(0, 0, idx[np.lexsort((idx, xy[:, 0]))], idx[np.lexsort((idx, xy[:, 1]))])]
    while stack:
        lo, depth, lx, ly = stack.pop()
        n = len(lx)
        if n == 0:
            continue
        a = depth & 1
        A, O = (lx, ly) if a == 0 else (ly, lx)
        k = (n - 1) // 2
        key = xy[A[k], a]
        if (k > 0 and xy[A[k - 1], a] == key) or (k + 1 < n and xy[A[k + 1], a] == key):
            ambiguous = True
            if not force:
                return None, True
        perm[lo + k] = A[k]
        rank[A] = np.arange(n)
        r = rank[O]
        left = (A[:k], O[r < k]) if a == 0 else (O[r < k], A[:k])
        right = (A[k + 1:], O[r > k]) if a == 0 else (O[r > k], A[k + 1:])
        stack.append((lo, depth + 1) + left)
        stack.append((lo + k + 1, depth + 1) + right)
    return perm, ambiguous


def ambiguous(xy):
    return build_sorted(xy)[1]


def tree_order(xy, perm):
    return np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2)[perm])
