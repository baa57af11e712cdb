"""Depth maps and queries for the keyframe's depth association (KeyFrame::setDepthMap, KeyFrame.cpp:1137-1166) — test helpers.

The reference finds each candidate's nearest depth-map point with its k-d tree (src/utils/KDTree.hpp); ties are decided by the tree's
traversal.  Real depth maps tie all the time: IDepthMap2d::fromDepthmapImage / fromDistanceImage (src/mapping/Types.hpp:153-232)
insert integer pixels column by column (x outer, y inner) and skip NaN holes, and the queries are integer pixels.  The helpers here
build such maps, and real-valued clouds with constructed near-ties whose winner depends on how dx*dx + dy*dy is rounded.

Golden files (tests/golden/kdtree/ref_kdtree_*.npz, written by tests/golden/make_ref_kdtree_golden.py from the reference's own tree) hold
    depth_xy   float64 m x 2 — or, for pixel grids, H, W and mask (np.packbits of the H x W row-major mask of depth pixels),
               expanded column-major by grid_points()
    queries    float64 n x 2 — or, when absent, every integer pixel of the H x W frame, row-major (query y * W + x)
    ref_idx    int32 n: the index KDTree::nnSearch returns;   ref_dist  float64 n: its minDist
"""
import glob
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kdtree")


def grid_points(mask):
    """fromDepthmapImage's insertion order: x outer, y inner, holes (False) skipped.  Returns float64 m x 2 (x, y)."""
    ys, xs = np.nonzero(np.asarray(mask, dtype=bool).T)[::-1]        # nonzero of the transpose walks x outer, y inner
    return np.stack([xs, ys], axis=1).astype(np.float64)


def frame_queries(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)


def holes_mask(rng, H, W, holes=0.15, block=None, step=1):
    """Depth at every `step`-th pixel, `holes` of them NaN at random, plus one rectangular hole `block` = (h, w) if given."""
    m = np.zeros((H, W), dtype=bool)
    m[::step, ::step] = True
    m &= rng.random((H, W)) >= holes
    if block is not None:
        bh, bw = block
        y0, x0 = int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1))
        m[y0:y0 + bh, x0:x0 + bw] = False
    return m


def depth_image_map(rng, H, W, holes=0.15, block=None, step=1):
    """A depth map shaped like fromDepthmapImage's: (depth_xy, idp) with idp distinct per point."""
    xy = grid_points(holes_mask(rng, H, W, holes, block, step))
    return xy, rng.uniform(0.2, 1.0, len(xy))


def load(name):
    """A golden case: dict with depth_xy, queries, ref_idx, ref_dist (and H, W for pixel-grid cases)."""
    g = np.load(os.path.join(GOLDEN, name))
    out = {k: g[k] for k in g.files}
    if "mask" in g.files:
        H, W = int(g["H"]), int(g["W"])
        out["mask_image"] = np.unpackbits(g["mask"], count=H * W).reshape(H, W).astype(bool)
        out["depth_xy"] = grid_points(out["mask_image"])
    if "queries" not in g.files:
        out["queries"] = frame_queries(int(g["H"]), int(g["W"]))
    out["ref_idx"] = out["ref_idx"].astype(np.int64)
    return out


def golden_names():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ref_kdtree_*.npz")))


# ---- near ties --------------------------------------------------------------------------------------------------------
def _d2_separate(q, t):
    dx, dy = q[0] - t[0], q[1] - t[1]
    return (0.0 + dx * dx) + dy * dy                 # KDTree::distance: every product and sum rounded on its own (numpy: no FMA)


def _d2_contracted(q, t):
    dx, dy = q[0] - t[0], q[1] - t[1]
    return float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))    # fma(dy, dy, dx*dx): `dist += dy*dy` contracted


def near_tie_pair(rng, q, kind, radius=(0.4, 1.0), tries=200000):
    """Two points about the query q whose order in sqrt distance is a near-tie of the given kind:
    'fma'   — the order of sqrt(dx*dx + dy*dy) with separate rounding is strict and contracting `+ dy*dy` into an FMA reverses it;
    'sqrt'  — distinct squared distances that round to the same sqrt (a tie for the tree, not for a squared-distance search);
    'swap'  — the same offset with x and y swapped: an exact tie with separate rounding, a strict order once contracted."""
    q = np.asarray(q, dtype=np.float64)
    for _ in range(tries):
        r, th = rng.uniform(*radius), rng.uniform(0, 2 * np.pi)
        a = q + np.array([r * np.cos(th), r * np.sin(th)])
        sa = _d2_separate(q, a)
        if kind == "swap":
            b = q + np.array([a[1] - q[1], a[0] - q[0]])
        else:                                                    # a second point on the same circle, to the nearest coordinate
            x = q[0] + rng.uniform(-1, 1) * np.sqrt(sa) * 0.9
            b = np.array([x, q[1] + np.sqrt(sa - (q[0] - x) ** 2) * rng.choice([-1.0, 1.0])])
        sb = _d2_separate(q, b)
        ra, rb = np.sqrt(sa), np.sqrt(sb)
        ca, cb = np.sqrt(_d2_contracted(q, a)), np.sqrt(_d2_contracted(q, b))
        if kind == "sqrt" and sa != sb and ra == rb:
            return a, b
        if kind == "fma" and ra != rb and ca != cb and (ra < rb) != (ca < cb):
            return a, b
        if kind == "swap" and ra == rb and ca != cb:
            return a, b
    raise RuntimeError(f"no {kind} near-tie about {q} in {tries} tries")


def near_tie_lattice(rng, H, W, spacing, kind, margin=2):
    """A pair of near-tie points (near_tie_pair) about every integer site of a lattice over an H x W frame, shuffled pairwise.
    Returns (depth_xy 2s x 2, sites s x 2): the pair of site k is depth_xy[2k], depth_xy[2k + 1], in random order."""
    sites = np.array([(x, y) for y in range(margin, H - margin, spacing) for x in range(margin, W - margin, spacing)], dtype=np.float64)
    pts = []
    for s in sites:
        a, b = near_tie_pair(rng, s, kind)
        pts.extend([a, b] if rng.random() < 0.5 else [b, a])
    return np.asarray(pts), sites


def contracted_winner(depth_xy, q, cand):
    """Among the candidate indices, the one a search with `dist += dy*dy` contracted into an FMA would prefer (strictly nearer)."""
    d = [np.sqrt(_d2_contracted(q, depth_xy[i])) for i in cand]
    return cand[int(np.argmin(d))]
