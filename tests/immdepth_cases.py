"""The cases of tests/test_immdepth_oracle.py and tests/test_immdepth_gpu.py: a 64 x 48 textured image, a depth map (x, y in fp64 and
inverse depths) and a pixel list per case.  Every case is generated from a fixed seed; nothing here computes an expected value."""
import functools

import numpy as np

H, W = 48, 64
SIZES = (1, 2, 3, 63, 64, 65, 1000, 4096, 4097)           # random real-valued maps
LIST_SIZES = (1, 63, 64, 65, 256, 257, 1000)              # pixel lists through eds_imd_create_points: one block, its edges, several blocks


class Case:
    def __init__(self, name, xy, idp, uv, typ, scale=None, ties=False):
        self.name, self.image = name, image()
        self.xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self.idp = np.ascontiguousarray(idp, dtype=np.float64).reshape(-1)
        self.uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
        self.type = np.ascontiguousarray(typ, dtype=np.float32)
        self.scale, self.ties = scale, ties              # ties: some pixel has two nearest points at exactly the same distance


@functools.lru_cache(maxsize=None)
def image():
    """fp32 intensities 0 .. 255 with gradients everywhere, so that a pixel selector selects all over it"""
    r = np.random.default_rng(20240)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 128 + 50 * np.sin(0.37 * x + 0.11 * y) * np.cos(0.23 * y - 0.05 * x) + 30 * r.standard_normal((H, W))
    return np.clip(img, 0, 255).astype(np.float32)


def pixels(n, seed):
    """n distinct pixels in row-major order, the image border included (their pattern leaves the image), and their my_type"""
    r = np.random.default_rng(seed)
    flat = np.sort(r.choice(H * W, size=n, replace=False))
    uv = np.stack([flat % W, flat // W], axis=1).astype(np.int32)
    return uv, r.choice(np.array([1, 2, 4], np.float32), size=n)


def random_map(m, seed, w=W, h=H):
    r = np.random.default_rng(seed)
    xy = np.stack([r.uniform(0, w, m), r.uniform(0, h, m)], axis=1)
    return xy, r.uniform(0.05, 2.0, m)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for m in SIZES:
        xy, idp = random_map(m, 100 + m)
        uv, typ = pixels(300, 200 + m)
        out[f"random_{m}"] = Case(f"random_{m}", xy, idp, uv, typ)
    # an integer-pixel grid: every axis value occurs many times, so the map is ambiguous and the host builds its tree
    gy, gx = np.mgrid[0:H:2, 0:W:2]
    gxy = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float64)
    uv, typ = pixels(300, 31)
    out["grid"] = Case("grid", gxy, np.random.default_rng(32).uniform(0.05, 2.0, len(gxy)), uv, typ, ties=True)
    # exact ties: map points at (u - 0.5, v) and (u + 0.5, v) around pixels of the list, with distinct inverse depths
    uv, typ = pixels(120, 41)
    centres = uv[::3].astype(np.float64)
    txy = np.concatenate([centres + [-0.5, 0.0], centres + [0.5, 0.0], random_map(40, 42)[0]])
    out["ties"] = Case("ties", txy, np.random.default_rng(43).uniform(0.05, 2.0, len(txy)), uv, typ, ties=True)
    # a neighbour at exactly 1.0 (GOOD: the reference tests > 1.0) and one ulp of the coordinate above (UNINITIALIZED); the pixels lie
    # far apart and far from the other points, so each has its one neighbour
    uv = np.array([[10, 10], [30, 10], [50, 10], [10, 30], [30, 30], [50, 30]], np.int32)
    nb = np.array([[11.0, 10.0], [np.nextafter(31.0, 64.0), 10.0], [50.0, 11.0], [10.0, np.nextafter(31.0, 64.0)], [29.0, 30.0],
                   [50.0, np.nextafter(29.0, 0.0)]])
    out["distance_one"] = Case("distance_one", nb, np.array([0.5, 0.6, 0.7, 0.8, 0.9, 1.0]), uv, np.ones(6, np.float32))
    # a scale: the query is scaled into the map's frame, the distance is taken against the unscaled pixel
    xy, idp = random_map(500, 51, W * 0.5, H * 0.25)
    uv, typ = pixels(300, 52)
    out["scaled"] = Case("scaled", xy, idp, uv, typ, scale=(0.5, 0.25))
    # negative and NaN inverse depths ride through unchanged
    xy, idp = random_map(1500, 61)
    idp[::3] = -idp[::3]
    idp[1::7] = np.nan
    uv, typ = pixels(300, 62)
    out["odd_idepth"] = Case("odd_idepth", xy, idp, uv, typ)
    uv, typ = pixels(300, 71)
    out["empty"] = Case("empty", np.zeros((0, 2)), np.zeros(0), uv, typ)
    return out
