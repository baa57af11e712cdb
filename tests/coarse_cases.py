"""Seeded cases for the coarse tracker (include/eds_hip_coarse.h): a smooth textured plane seen from two poses a known small SE(3) apart,
so the new image is the reference image under the plane's homography, exactly; the contributions are pixels of the reference frame
with the plane's inverse depth.  The shapes are the smallest at which the kernels can still go wrong: 64 x 48 with 3 levels and
96 x 64 with 4, fx != fy, an off-centre principal point, level-0 lists that are no multiple of 4, 32 or 512 and one longer than 512,
several contributions on one pixel, contributions on the border and off the image, a level whose list is empty, a try that sends
every point out of bounds, a brightness jump that forces the cutoff doubling and the level repeat, the four affineOptMode
combinations and a try that aborts on minResForAbort."""
import functools
import types

import numpy as np


def texture(x, y):
    return (128.0 + 45.0 * np.sin(0.21 * x + 0.09 * y) + 35.0 * np.cos(0.12 * y - 0.05 * x) + 18.0 * np.sin(0.043 * x + 0.3)
            * np.cos(0.057 * y) + 9.0 * np.sin(0.5 * x - 0.37 * y))


def se3(rotvec, t):
    """3 x 4 [R | t] from a rotation vector (Rodrigues) and a translation"""
    w = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
    return np.concatenate([R, np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1)


def _plane_idepth(K, n, d, u, v):
    fx, fy, cx, cy = K
    return (n[0] * (u - cx) / fx + n[1] * (v - cy) / fy + n[2]) / d


def make(seed, H, W, levels, K, n_points, motion, gain=(0.0, 0.0), prm=None, tries=None, aff_init=None, coarsest=None, min_res=None,
         exposures=(1.0, 1.0), aff_ref=(0.0, 0.0), columns=None, dup=0.15, stray=8):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    n, d = np.array([0.08, -0.05, 1.0]), 2.0                   # the plane n . X = d in the reference frame
    T = se3(*motion)
    Hom = Km @ (T[:, :3] + np.outer(T[:, 3], n) / d) @ np.linalg.inv(Km)          # reference pixel -> new pixel
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ref = texture(xx, yy)
    back = np.linalg.inv(Hom) @ np.stack([xx.ravel(), yy.ravel(), np.ones(H * W)])
    new = texture(back[0] / back[2], back[1] / back[2]).reshape(H, W)
    new = np.exp(gain[0]) * new + gain[1]
    # contributions: seeded pixels (a share of them twice or three times, with their own idepth noise and HdiF), sub-pixel offsets
    lo, hi = (0, W) if columns is None else columns
    u = rng.integers(lo, hi, n_points).astype(np.float64)
    v = rng.integers(0, H, n_points).astype(np.float64)
    k = int(dup * n_points)
    src = rng.integers(0, n_points, k)
    u[n_points - k:], v[n_points - k:] = u[src], v[src]
    order = rng.permutation(n_points)
    u, v = u[order], v[order]
    idp = _plane_idepth(K, n, d, u, v) * (1.0 + 0.01 * rng.standard_normal(n_points))
    cp = np.stack([u + rng.uniform(-0.45, 0.45, n_points), v + rng.uniform(-0.45, 0.45, n_points), idp], axis=1)
    hdif = rng.uniform(0.5, 400.0, n_points)
    if stray:                                                  # on the border, just inside, just outside, far outside
        xs = np.array([-0.6, -0.4, W - 0.6, W - 0.4, 3.0, 3.0, -40.0, 1e9])[:stray]
        ys = np.array([5.0, 5.0, 7.0, 7.0, -0.6, H - 0.4, 9.0, 9.0])[:stray]
        at = np.linspace(3, n_points - 3, stray).astype(int)
        cp[at, 0], cp[at, 1] = xs, ys
    c = types.SimpleNamespace(H=H, W=W, levels=levels, K=tuple(np.float32(K).tolist()), prm=dict(prm or {}), ref=ref.astype(np.float32),
                              new=new.astype(np.float32), cp=cp.astype(np.float32), hdif=hdif.astype(np.float32),
                              exposure_ref=exposures[0], exposure_new=exposures[1], aff_ref=aff_ref, T_true=T)
    c.T_init = np.stack(tries if tries is not None else [se3((0, 0, 0), (0, 0, 0))])
    c.aff_init = np.zeros((len(c.T_init), 2)) if aff_init is None else np.asarray(aff_init, dtype=np.float64)
    c.coarsest = levels - 1 if coarsest is None else coarsest
    c.min_res = np.full(5, np.nan) if min_res is None else np.asarray(min_res, dtype=np.float64)
    return c


IDENT = se3((0, 0, 0), (0, 0, 0))
SMALL = ((0.004, -0.006, 0.01), (0.02, -0.012, 0.008))
K64 = (58.0, 61.5, 30.3, 25.1)
K96 = (85.0, 80.0, 49.6, 30.2)


@functools.lru_cache(maxsize=None)
def cases():
    far = se3((0, 0, 0), (50.0, 0, 0))                          # every point leaves the image: numTermsInE == 0
    near = se3((0.002, 0.001, -0.004), (0.01, 0.0, 0.0))
    c = {}
    c["a64_l3"] = make(1, 48, 64, 3, K64, 700, SMALL, tries=[IDENT, near, far])
    c["b96_l4"] = make(2, 64, 96, 4, K96, 1500, SMALL, gain=(0.05, 4.0), tries=[IDENT, near], exposures=(0.9, 1.1), aff_ref=(0.02, -1.5))
    c["jump"] = make(3, 48, 64, 3, K64, 500, SMALL, gain=(0.0, 70.0))                       # cutoff doubling, one level repeated
    c["empty_top"] = make(4, 48, 64, 3, K64, 60, SMALL, columns=(2, 4), stray=0)           # level 2's list is empty
    c["abort"] = make(5, 48, 64, 3, K64, 300, SMALL, min_res=[1e-3] * 5)
    for i, (ma, mb) in enumerate(((-1.0, -1.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 0.0))):
        c[f"mode_{i}"] = make(6 + i, 48, 64, 3, K64, 110 + 3 * i, SMALL, gain=(0.03, 2.0), prm=dict(affine_opt_mode_a=ma, affine_opt_mode_b=mb))
    return c


# the cases whose whole loop is compared between the oracle, g++ and the device
LOOP_CASES = ("a64_l3", "b96_l4", "jump", "empty_top", "abort", "mode_0", "mode_1", "mode_2", "mode_3")
