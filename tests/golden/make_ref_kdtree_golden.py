"""Regenerates tests/golden/kdtree/ref_kdtree_*.npz from the reference's own k-d tree (oracle/_ref/kdtree_nn: src/utils/KDTree.hpp,
unmodified, built by oracle/ref/Makefile with the reference's flags).  Each file holds a case's inputs — pixel grids as packed masks,
real-valued points as float64 — and the reference's nnSearch index and minDist for every query (layout: tests/kdtree_cases.py).
Where the reference tree is absent, prints so and changes nothing.

    python tests/golden/make_ref_kdtree_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref"))
sys.path.insert(0, os.path.dirname(HERE))
import kdtree_cases as kc  # noqa: E402
import refcase  # noqa: E402


def cases():
    rng = np.random.default_rng(20261016)
    for name, (H, W, step, block) in {"dense_120x160": (120, 160, 1, (19, 29)), "dense_61x83": (61, 83, 1, (11, 17)),
                                       "every_other_120x160": (120, 160, 2, None)}.items():
        mask = kc.holes_mask(rng, H, W, 0.15, block, step)
        yield name, dict(H=H, W=W, mask=np.packbits(mask.ravel())), kc.grid_points(mask), kc.frame_queries(H, W)
    g = np.array([(x, y) for y in range(0, 8, 2) for x in range(0, 8, 2)], dtype=np.float64)     # 4 x 4 at even coordinates
    q = np.array([(1, 1), (3, 1), (1, 3), (3, 3), (2, 2), (7, 7), (-1, -1)], dtype=np.float64)
    yield "grid4x4_row_major", dict(depth_xy=g, queries=q), g, q
    gc = g.reshape(4, 4, 2).transpose(1, 0, 2).reshape(-1, 2).copy()                                 # the same, column by column
    yield "grid4x4_col_major", dict(depth_xy=gc, queries=q), gc, q
    base = kc.grid_points(kc.holes_mask(rng, 30, 40, 0.3))
    dup = np.concatenate([base, base[rng.permutation(len(base))[:len(base) // 2]], base[:50]])       # ties at distance 0
    dup = dup[rng.permutation(len(dup))]
    yield "duplicates", dict(H=30, W=40, depth_xy=dup), dup, kc.frame_queries(30, 40)
    row = np.stack([np.arange(0, 90, 3.0), np.full(30, 7.0)], axis=1)
    col = np.stack([np.full(30, 5.0), np.arange(0, 60, 2.0)], axis=1)
    yield "single_row", dict(H=15, W=92, depth_xy=row), row, kc.frame_queries(15, 92)
    yield "single_column", dict(H=62, W=12, depth_xy=col), col, kc.frame_queries(62, 12)
    tiny = []
    for m in (1, 2, 3, 4):
        for t in range(4):
            p = rng.integers(0, 6, (m, 2)).astype(np.float64)
            tiny.append(p)
    qs = kc.frame_queries(8, 8) - 1.0                                          # -1 .. 6: outside the hull too
    for k, p in enumerate(tiny):
        yield f"tiny_m{len(p)}_{k % 4}", dict(depth_xy=p, queries=qs), p, qs
    p = rng.integers(0, 24, (300, 2)).astype(np.float64)
    p = p[rng.permutation(len(p))]
    qs = np.array([(x, y) for x in np.unique(p[:, 0]) for y in np.unique(p[:, 1])] +                 # on split planes
                  [(x, y) for x in (-30.0, -5.0, 12.5, 40.0, 1e3) for y in (-7.0, 11.5, 30.0, -1e3)])    # and outside the hull
    yield "split_planes_and_outside", dict(depth_xy=p, queries=qs), p, qs
    for kind in ("fma", "sqrt", "swap"):
        xy, sites = kc.near_tie_lattice(rng, 60, 80, 6, kind)
        yield f"near_tie_{kind}", dict(H=60, W=80, depth_xy=xy, queries=sites), xy, sites


if __name__ == "__main__":
    msg = refcase.build()
    if not refcase.kdtree_available():
        print(msg or "kdtree unpinned: oracle/_ref/kdtree_nn was not built")
        sys.exit(0)
    for name, store, xy, q in cases():
        idx, dist = refcase.kdtree_nn(xy, q)
        path = os.path.join(HERE, "kdtree", f"ref_kdtree_{name}.npz")
        np.savez_compressed(path, ref_idx=idx.astype(np.int32), ref_dist=dist, **store)
        print(f"wrote {os.path.basename(path)}: m = {len(xy)}, {len(q)} queries, {os.path.getsize(path)} bytes")
