"""Depth maps of the k-d build tests (include/eds_hip_kfswitch.h), shared by the CPU tests (tests/test_kdbuild_oracle.py), which assert
on the oracle alone what each case is, and the GPU tests (tests/test_kfswitch_gpu.py).  Pure numpy: the same bytes on every machine."""
import numpy as np

import np_kdbuild_oracle as kd

CAPACITY = 4096                         # eds_kfs_tree_capacity(); the CPU test checks the header's constant against it
SIZES = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1000, CAPACITY)


def real_map(seed, m, H=61, W=83):
    rng = np.random.default_rng([0x6B64, seed, m])
    return np.column_stack([rng.uniform(0, W, m), rng.uniform(0, H, m)])


def planted_away(seed, m=200):
    """a real-valued map with duplicated x and y values that never meet a median: pairs are drawn until the oracle says unambiguous"""
    rng = np.random.default_rng([0x6475, seed])
    for _ in range(1000):
        xy = real_map(1000 + seed, m)
        for axis in (0, 1):
            i, j = rng.choice(m, size=2, replace=False)
            xy[j, axis] = xy[i, axis]
        if not kd.ambiguous(xy):
            return xy
    raise AssertionError("no unambiguous planted map found")


def projected_maps():
    """the maps k_kfp_project's numpy oracle gives for the projection cases of tests/kfpoints_cases.py (projected to the slot's own size
    and to another one)"""
    import kfpoints_cases as kc
    import np_kfpoints_oracle as kp
    out = []
    for case in kc.projection_cases():
        ref = kp.project(**kc.projection_inputs(case))
        out.append(("projected-" + case[0], np.ascontiguousarray(ref["xy"])))
    return out


def dyadic_map(seed=5, m=300, H=61, W=83):
    """coordinates that are multiples of 2^-10: midpoints, differences, squares and their sums are exact in fp64, so the midpoint of two
    points is at EXACTLY the same distance from both"""
    rng = np.random.default_rng([0x6479, seed])
    return np.column_stack([rng.integers(0, W * 1024, m), rng.integers(0, H * 1024, m)]) / 1024.0


def unambiguous_cases():
    out = [(f"real-{m}", real_map(m, m)) for m in SIZES] + [("dyadic-300", dyadic_map())]
    out += [(f"planted-away-{s}", planted_away(s)) for s in range(3)]
    return out + projected_maps()


def integer_grid(seed, H=23, W=31, keep=0.6):
    rng = np.random.default_rng([0x6772, seed])
    ys, xs = np.mgrid[0:H, 0:W]
    pts = np.column_stack([xs.ravel(), ys.ravel()]).astype(np.float64)
    return pts[rng.random(len(pts)) < keep]


def _dup_of_median(xy, lo_set, axis, victim_rank):
    """copies the axis value of lo_set's median (rank (n - 1) // 2 on `axis`) to its element of rank victim_rank"""
    order = lo_set[np.argsort(xy[lo_set, axis], kind="stable")]
    xy = xy.copy()
    xy[order[victim_rank], axis] = xy[order[(len(order) - 1) // 2], axis]
    return xy


def ambiguous_cases():
    base = real_map(77, 101)
    order_x = np.argsort(base[:, 0], kind="stable")
    left = order_x[:50]                                 # the root's left side: the inner node of level 1 splits it on y
    zeros = np.array([[-2.0, 0.1], [-1.0, 0.7], [-0.0, 0.3], [0.0, 0.9], [3.0, 0.5]])
    nan, inf = real_map(78, 40), real_map(79, 40)
    nan[17, 1] = np.nan
    inf[3, 0] = np.inf
    out = [(f"grid-holes-{s}", integer_grid(s)) for s in range(4)]
    out += [("single-row", np.column_stack([np.arange(37.0), np.full(37, 5.0)])),
            ("single-column", np.column_stack([np.full(29, 7.0), np.arange(29.0)])),
            ("dup-root-median", _dup_of_median(base, np.arange(101), 0, 80)),
            ("dup-inner-median", _dup_of_median(base, left, 1, 40)),
            ("signed-zero-median", zeros),
            ("nan", nan), ("inf", inf)]
    return out


def tie_queries(xy, seed, n=40):
    """n midpoints of a map point and its nearest neighbour (exact distance ties where the arithmetic is exact: dyadic_map), then n
    random queries"""
    rng = np.random.default_rng([0x7469, seed])
    xy = np.asarray(xy)
    i = rng.integers(0, len(xy), n)
    d = ((xy[i, None, :] - xy[None]) ** 2).sum(-1)
    d[np.arange(n), i] = np.inf
    mid = (xy[i] + xy[np.argmin(d, axis=1)]) / 2.0
    return np.concatenate([mid, np.column_stack([rng.uniform(-5, 90, n), rng.uniform(-5, 70, n)])])


# -- the keyframe builds of tests/test_kfswitch_gpu.py ----------------------------------------------------------------------------------
def image(seed, H, W, dtype=np.float32):
    rng = np.random.default_rng([0x696D, seed])
    img = rng.standard_normal((H, W))
    for _ in range(3):
        img = (img + np.roll(img, 1, 0) + np.roll(img, 1, 1) + np.roll(img, -1, 0) + np.roll(img, -1, 1)) / 5.0
    img = (img - img.min()) / (img.max() - img.min())
    if dtype == np.uint8:
        return np.round(img * 255.0).astype(np.uint8)
    return img.astype(dtype)


def keyframe_map(seed, H, W, m=300):
    """a real-valued map with a region without support, so that cleanPoints drops points; (xy, idp)"""
    rng = np.random.default_rng([0x6D70, seed])
    xy = np.column_stack([rng.uniform(0, W - 1, m), rng.uniform(0, H - 1, m)])
    xy = xy[~((xy[:, 0] > 0.6 * W) & (xy[:, 1] > 0.5 * H))]
    return xy, rng.uniform(0.3, 1.0, len(xy))


def keyframe_grid_map(seed, H, W):
    xy = integer_grid(seed, H, W, keep=0.3)
    return xy, np.random.default_rng([0x6770, seed]).uniform(0.3, 1.0, len(xy))


FRAMES = ((61, 83), (83, 61))
KEYFRAME_MAP_SEEDS = tuple(range(20))    # every real-valued keyframe map of the GPU tests: keyframe_map(s, H, W) for these seeds and FRAMES


def device_built_maps():
    """every map the GPU tests expect the DEVICE to build: the CPU test checks each is unambiguous and within the capacity"""
    out = unambiguous_cases()
    for H, W in FRAMES:
        out += [(f"keyframe-{H}x{W}-{s}", keyframe_map(s, H, W)[0]) for s in KEYFRAME_MAP_SEEDS]
    return out
