"""Seeded cases for the initialiser (include/eds_hip_init.h), built from tests/coarse_cases.py's texture, se3 and plane: a first frame and
a sequence of frames along a growing motion, each the first frame under the plane's homography, exactly.  Status maps come from a
gradient threshold (level 0, and level 1 where there is one above it) and full density (the top level); the tables are the exact
10-nearest / 1-nearest ones with ties to the lower index, formed here in numpy.

  a96    96 x 80, 3 levels: level 0 has between 513 and 1 023 points and no multiple of 64; the top level is at full density, so optReg
         and resetPoints have long dependency chains; six frames whose |t| passes 0.0167 in the first frame's units (idepth 1), where
         alphaW |t|^2 npts exceeds alphaK npts and `snapped` becomes possible.
  b64    64 x 48, 2 levels, fix_affine = 0, a gain change between the frames and both exposures positive: the 8 x 8 solve, the logf guess.
  edges  a96 with a pose guess that pushes a band of points out of the image, neighbour entries of -1, and points with at most two
         good neighbours: bad points, the nnn <= 2 branch, resetPoints' revival.
"""
import functools
import types

import numpy as np

import coarse_cases as cc

PLANE_N, PLANE_D = np.array([0.08, -0.05, 1.0]), 2.0


def frame_at(H, W, K, T, gain=(0.0, 0.0)):
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Hom = Km @ (T[:, :3] + np.outer(T[:, 3], PLANE_N) / PLANE_D) @ np.linalg.inv(Km)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    back = np.linalg.inv(Hom) @ np.stack([xx.ravel(), yy.ravel(), np.ones(H * W)])
    img = cc.texture(back[0] / back[2], back[1] / back[2]).reshape(H, W)
    return (np.exp(gain[0]) * img + gain[1]).astype(np.float32)


def pyramid_colour(img, levels):
    out = [np.asarray(img, dtype=np.float32)]
    for _ in range(1, levels):
        p = out[-1]
        out.append(np.float32(0.25) * (((p[0::2, 0::2] + p[0::2, 1::2]) + p[1::2, 0::2]) + p[1::2, 1::2]))
    return out


def gradient_status(colour, share):
    """1 where the squared gradient is in the upper `share` of the level, 0 elsewhere"""
    gx = np.zeros_like(colour); gy = np.zeros_like(colour)
    gx[:, 1:-1] = 0.5 * (colour[:, 2:] - colour[:, :-2])
    gy[1:-1, :] = 0.5 * (colour[2:, :] - colour[:-2, :])
    g2 = gx * gx + gy * gy
    return (g2 > np.quantile(g2, 1.0 - share)).astype(np.float32)


def rect_points(status):
    """(u, v) of the points a status map gives, in the order of setFirst's loop"""
    h, w = status.shape
    ys, xs = np.nonzero(status[3:h - 4, 3:w - 4])
    return np.stack([(xs + 3 + 0.1).astype(np.float32), (ys + 3 + 0.1).astype(np.float32)], axis=1)


def exact_nn(uv, uv_up):
    """the 10 nearest by (fp32 squared distance, index), and the nearest of the level above to 0.5 pt - 0.25"""
    uv = np.asarray(uv, dtype=np.float32)
    d0 = uv[:, None, 0] - uv[None, :, 0]; d1 = uv[:, None, 1] - uv[None, :, 1]
    d = d0 * d0 + d1 * d1
    nb = np.argsort(d, axis=1, kind="stable")[:, :10].astype(np.int32)
    if nb.shape[1] < 10:
        nb = np.concatenate([nb, np.full((len(uv), 10 - nb.shape[1]), -1, np.int32)], axis=1)
    if uv_up is None:
        return nb, None
    q = uv * np.float32(0.5) - np.float32(0.25)
    e0 = q[:, None, 0] - uv_up[None, :, 0]; e1 = q[:, None, 1] - uv_up[None, :, 1]
    return nb, np.argmin(e0 * e0 + e1 * e1, axis=1).astype(np.int32)


def make(seed, H, W, levels, K, step, n_frames, share0, prm=None, gains=None, exposures=None, pose_guess=None, holes=False):
    rng = np.random.default_rng(seed)
    c = types.SimpleNamespace(H=H, W=W, levels=levels, K=tuple(np.float32(K).tolist()), prm=dict(prm or {}), pose_guess=pose_guess, cap=4096)
    c.first = frame_at(H, W, K, cc.se3((0, 0, 0), (0, 0, 0)))
    c.T_true = [cc.se3(np.multiply(step[0], k), np.multiply(step[1], k)) for k in range(1, n_frames + 1)]
    gains = gains or [(0.0, 0.0)] * n_frames
    c.frames = [frame_at(H, W, K, T, g) for T, g in zip(c.T_true, gains)]
    c.exposures = exposures or [1.0] * (n_frames + 1)
    colour = pyramid_colour(c.first, levels)
    c.status = [gradient_status(colour[l], share0 if l == 0 else 0.5) if l < levels - 1 else np.ones_like(colour[l]) for l in range(levels)]
    c.status[0] *= rng.choice(np.float32([1.0, 2.0, 4.0]), size=c.status[0].shape)             # my_type as the selector would give it
    c.uv = [rect_points(s) for s in c.status]
    c.nb, c.parent = [], []
    for l in range(levels):
        nb, par = exact_nn(c.uv[l], c.uv[l + 1] if l + 1 < levels else None)
        if holes:                                            # -1 entries, and a few points left with at most two neighbours
            nb = nb.copy()
            nb[rng.random(nb.shape) < 0.08] = -1
            for i in rng.choice(len(nb), size=max(3, len(nb) // 40), replace=False):
                nb[i, rng.permutation(10)[:rng.integers(8, 11)]] = -1
        c.nb.append(nb); c.parent.append(par)
    return c


K96 = (85.0, 80.0, 49.6, 40.2)
K64 = (58.0, 61.5, 30.3, 25.1)
STEP = ((0.002, -0.003, 0.004), (0.016, -0.009, 0.006))


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["a96"] = make(11, 80, 96, 3, K96, STEP, 6, 0.12)
    c["b64"] = make(12, 48, 64, 2, K64, STEP, 4, 0.3, prm=dict(fix_affine=0), gains=[(0.04 * k, 1.5 * k) for k in range(1, 5)],
                    exposures=[0.8, 0.9, 1.0, 1.1, 1.25])
    c["edges"] = make(11, 80, 96, 3, K96, STEP, 6, 0.12, pose_guess=cc.se3((0.0, 0.07, 0.0), (0, 0, 0)), holes=True)
    return c
