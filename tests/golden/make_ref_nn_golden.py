"""Regenerates tests/golden/nn/ref_nn_*.npz from the reference's own nanoflann (oracle/_ref/nanoflann_nn: src/utils/nanoflann.h,
unmodified, built by oracle/ref/Makefile with the reference's flags and called as CoarseInitializer::makeNN calls it).  Each file holds a
case's points, the points of the level above, and the reference's neighbour and parent tables with their squared distances (layout:
tests/nn_cases.py).  Every case comes from a fixed seed.  Where the reference tree is absent, prints so and changes nothing.

    python tests/golden/make_ref_nn_golden.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref"))
sys.path.insert(0, os.path.dirname(HERE))
import nn_cases as nc  # noqa: E402
import np_nn_oracle as nno  # noqa: E402
import refcase  # noqa: E402

MAX_BYTES = 39455                # the largest file of tests/golden/kdtree/


def cases():
    """(name, uv, uv_up, (H, W) of the level for lattice cases or None)"""
    rng = np.random.default_rng(20261020)
    H, W = 32, 40
    up30 = nc.lattice_uv(nc.pick_mask(rng, H // 2, W // 2, 30))
    # point counts: a node of <= 5 points is a leaf, 6 is the first split, 10 / 11 fill the result set exactly / by one more
    for n in (1, 2, 5, 6, 9, 10, 11, 12, 63, 65, 257):
        yield f"count_{n:03d}", nc.lattice_uv(nc.pick_mask(rng, H, W, n)), up30, (H, W)
    # lattice + 0.1: a third of the 40 x 32 level's rectangle, the full rectangle, a row, a column, a window where x + 0.1 is inexact
    third = nc.rect_mask(H, W) & (rng.random((H, W)) < 1.0 / 3.0)
    yield "lattice_40x32_third", nc.lattice_uv(third), up30, (H, W)
    yield "lattice_full_33x25", nc.lattice_uv(nc.rect_mask(H, W)), nc.lattice_uv(nc.rect_mask(H // 2, W // 2)), (H, W)
    row = np.zeros((16, 96), dtype=bool); row[7, :] = True
    col = np.zeros((96, 16), dtype=bool); col[:, 6] = True
    yield "lattice_row", nc.lattice_uv(row), nc.lattice_uv(nc.pick_mask(rng, 8, 48, 9)), (16, 96)
    yield "lattice_column", nc.lattice_uv(col), nc.lattice_uv(nc.pick_mask(rng, 48, 8, 9)), (96, 16)
    yield "lattice_x8000", nc.lattice_uv(nc.pick_mask(rng, 32, 8192, 500, 8000, 8090)), nc.lattice_uv(nc.pick_mask(rng, 16, 4096, 120, 3995, 4050)), (32, 8192)
    # parents: a level above of 700 points, of one point, and one that covers a corner only (most queries outside its hull)
    low = nc.lattice_uv(nc.pick_mask(rng, 80, 96, 400))
    yield "parents_700", low, nc.lattice_uv(nc.pick_mask(rng, 40, 48, 700)), (80, 96)
    yield "parents_1", low[::4], nc.lattice_uv(nc.pick_mask(rng, 40, 48, 1)), (80, 96)
    yield "parents_outside_hull", low[::2], nc.lattice_uv(nc.pick_mask(rng, 40, 48, 40, 3, 12)), (80, 96)
    # the host function only (level points are always lattice points): the split's lim1 / lim2 / count/2 fallback, real-valued
    # clouds, a tree deeper than the explicit walk's stack, and near-ties that an FMA would decide the other way
    yield "identical_12", np.full((12, 2), 7.1, np.float32), np.full((3, 2), 3.3, np.float32), None
    base = nc.lattice_uv(nc.pick_mask(rng, 30, 40, 150))
    dup = np.concatenate([base, base[rng.permutation(len(base))[:75]], base[:20], base[:20]])
    yield "duplicated_cloud", dup[rng.permutation(len(dup))], base[rng.integers(0, len(base), 60)] * np.float32(0.5), None
    yield "random_uniform", rng.uniform(0, 60, (300, 2)).astype(np.float32), rng.uniform(-5, 20, (80, 2)).astype(np.float32), None
    yield "random_clusters", (rng.normal(0, 1, (350, 2)) * rng.choice([0.01, 1.0, 30.0], (350, 1)) + 100).astype(np.float32), \
        rng.normal(50, 20, (50, 2)).astype(np.float32), None
    deep = np.stack([2.0 ** np.arange(-60, 60), np.zeros(120)], axis=1).astype(np.float32)
    yield "deep_tree", deep, deep[::-3].copy(), None
    uv, up = nc.near_tie_sites(rng, 8, 6)
    yield "near_tie_fma", uv, up, None


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed time stamp on every member, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    msg = refcase.build()
    if not refcase.nanoflann_available():
        print(msg or "makeNN unpinned: oracle/_ref/nanoflann_nn was not built")
        sys.exit(0)
    os.makedirs(os.path.join(HERE, "nn"), exist_ok=True)
    for name, uv, up, level in cases():
        r = refcase.nanoflann_nn(uv, up)
        store = dict(uv=np.asarray(uv, np.float32), uv_up=np.asarray(up, np.float32), ref_nb=r["nb"], ref_dist=r["dist"], ref_parent=r["parent"],
                     ref_parent_dist=r["parent_dist"])
        if level is not None:
            store.update(H=np.int32(level[0]), W=np.int32(level[1]))
        path = os.path.join(HERE, "nn", f"ref_nn_{name}.npz")
        save_npz(path, **store)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (name, size)
        ex = nno.exhaustive(uv)
        rows = int((ex != r["nb"]).any(axis=1).sum())
        sets = int((np.sort(ex, axis=1) != np.sort(r["nb"], axis=1)).any(axis=1).sum())
        print(f"wrote {os.path.basename(path)}: n = {len(uv)}, n_up = {len(up)}, {size} bytes; the exhaustive lower-index rule differs in "
              f"{rows} rows, {sets} of them as sets")
