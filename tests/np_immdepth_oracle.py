"""numpy statement of the loop of include/eds_hip_immdepth.h, written from the header's text and the reference (KDTree.hpp,
ImmaturePoint.cpp:68-114), independently of csrc/eds_immdepth.hpp:

    q = (u * scale[0], v * scale[1]);  k = nnSearch(q);  idepth = (float)map.idepth[k];
    distance = sqrt(dx * dx + dy * dy), dx = map.x[k] - u, dy = map.y[k] - v;  the second constructor.

Every operation is one fp64 numpy operation on arrays, so every product and sum is rounded on its own.  The nearest point is found by
brute force, which is the tree's answer only where the smallest sqrt distance occurs once: `unique` says where.  Where it does not, the
winner depends on the tree's shape and the traversal, and `walk` restates KDTree::nnSearch over a given index array (the tree that
tests/test_kdtree_pin.py pins to the reference's own)."""
import numpy as np

import np_immature_oracle as no

F = np.float32


def query(uv, scale=None):
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    sx, sy = (1.0, 1.0) if scale is None else (float(scale[0]), float(scale[1]))
    return np.stack([uv[:, 0].astype(np.float64) * sx, uv[:, 1].astype(np.float64) * sy], axis=1)


def _dist(a, b):
    """KDTree.hpp:253-259: sqrt(0 + dx dx + dy dy)"""
    dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
    return np.sqrt((0.0 + dx * dx) + dy * dy)


def brute(xy, uv, scale=None):
    """(index of the first smallest distance, unique): unique[i] is False where two map points share pixel i's smallest distance"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    q = query(uv, scale)
    d = _dist(q[:, None, :], xy[None, :, :])
    k = np.argmin(d, axis=1)
    dmin = d[np.arange(len(q)), k]
    return k, (d == dmin[:, None]).sum(axis=1) == 1


def walk(xy, perm, q):
    """KDTree::nnSearch (KDTree.hpp:99-112, :263-284) for one query over the tree `perm` (node of [lo, hi) at lo + (hi - lo - 1) // 2)"""
    best = [np.finfo(np.float64).max, int(perm[0])]

    def rec(lo, hi, depth):
        if lo >= hi:
            return
        mid = lo + (hi - lo - 1) // 2
        i = int(perm[mid])
        d = float(_dist(q, xy[i]))
        if d < best[0]:
            best[0], best[1] = d, i
        axis = depth % 2
        left = q[axis] < xy[i, axis]
        near, far = ((lo, mid), (mid + 1, hi)) if left else ((mid + 1, hi), (lo, mid))
        rec(near[0], near[1], depth + 1)
        if abs(q[axis] - xy[i, axis]) < best[0]:
            rec(far[0], far[1], depth + 1)

    rec(0, len(perm), 0)
    return best[1]


def winners(xy, uv, scale=None, perm=None):
    """the winner per pixel: brute force where it is unique, the pinned walk over `perm` elsewhere (perm None: unique is asserted)"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    k, unique = brute(xy, uv, scale)
    if not unique.all():
        assert perm is not None, "a tie needs the tree"
        q = query(uv, scale)
        for i in np.flatnonzero(~unique):
            k[i] = walk(xy, perm, q[i])
    return k.astype(np.int32), unique


def inputs(xy, idp, uv, k):
    """steps 3 and 4 for the winners k: (idepth float32, distance float64)"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    dx = xy[k, 0] - uv[:, 0].astype(np.float64)
    dy = xy[k, 1] - uv[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.asarray(idp, dtype=np.float64)[k].astype(F), np.sqrt(dx * dx + dy * dy)


def seed(image, xy, idp, uv, typ, scale=None, perm=None, prm=None):
    """the loop: (points as np_immature_oracle.construct returns them, dict(index, idepth, distance), unique)"""
    img = no.make_image(image)
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    n = len(uv)
    if len(np.asarray(xy).reshape(-1, 2)) == 0:
        nn = dict(index=np.full(n, -1, np.int32), idepth=np.zeros(n, F), distance=np.zeros(n))
        return no.construct(img, uv, typ, None, None, prm), nn, np.ones(n, bool)
    k, unique = winners(xy, uv, scale, perm)
    idepth, distance = inputs(xy, idp, uv, k)
    return no.construct(img, uv, typ, idepth, distance, prm), dict(index=k, idepth=idepth, distance=distance), unique
