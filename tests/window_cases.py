"""Seeded cases for the window optimiser's linearize (include/eds_hip_window.h): F views, a small known SE(3) apart, of one plane whose
texture has a smooth part, a FLAT part (no gradient: wJI2_sum < 2) and a patch of NaN pixels (a non-finite hitColor); every image is
that texture under the plane's homography, exactly.  Points are integer pixels of their host frame with the plane's inverse depth
plus noise, color[8] / weights[8] read from the host image as ImmaturePoint's constructor reads them.  64 x 48 images, fx != fy, an
off-centre principal point.  The shapes are the smallest at which the kernels can still go wrong: a single residual, a handful, 513
points in one host (one past the 512-lane stride) and 1 100 + 7 x 40 points over 8 frames with up to F - 1 residuals per point and a
(host, target) pair that has no residual at all.  Every branch occurs: entry state OOB, OOB from the centre projection (drescale <= 0,
and outside the image), OOB from a later tap, a non-finite colour, OUTLIER by energy and by wJI2_sum < 2, IN, both Huber branches,
affineOptMode negative and positive, a point with no active residual, a point clamped at 1e-10 (frame 1 is a pure rotation of frame
0: Jpdd is 0 between them), shiftPriorToZero 0 and 1."""
import functools
import types

import numpy as np

from coarse_cases import se3

f32 = np.float32
H, W = 48, 64
K = (58.0, 61.5, 30.3, 25.1)
PATTERN = ((0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2))
PLANE_N, PLANE_D = np.array([0.08, -0.05, 1.0]), 2.0
ENERGY_TH = 8 * 12.0 * 12.0                     # patternNum * setting_outlierTH


def texture(x, y):
    t = (128.0 + 45.0 * np.sin(0.21 * x + 0.09 * y) + 35.0 * np.cos(0.12 * y - 0.05 * x) + 18.0 * np.sin(0.043 * x + 0.3) * np.cos(0.057 * y)
         + 9.0 * np.sin(0.5 * x - 0.37 * y))
    t = np.where((x > 40.5) & (y < 15.5), 90.0, t)                       # flat
    return np.where((np.abs(x - 10.0) < 2.3) & (np.abs(y - 32.0) < 2.3), np.nan, t)


def _T44(T):
    return np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]])


def _precalc(Km, Th, Tt, T0h, T0t, aff_h, aff_t, exp_h, exp_t):
    """FrameFramePrecalc::set (HessianBlocks.cpp:204-234) as 27 floats"""
    K32, Ki32 = Km.astype(f32), np.linalg.inv(Km).astype(f32)
    ll0, ll = T0t @ np.linalg.inv(T0h), Tt @ np.linalg.inv(Th)
    R32, t32 = ll[:3, :3].astype(f32), ll[:3, 3].astype(f32)
    a = np.exp(aff_t[0] - aff_h[0]) * exp_t / exp_h
    b = aff_t[1] - a * aff_h[1]
    return np.concatenate([((K32 @ R32) @ Ki32).ravel(), K32 @ t32, ll0[:3, :3].ravel(), ll0[:3, 3], [a, b], [aff_h[1]]]).astype(f32)


def _adjoints(poses0, affs, exps):
    """EnergyFunctional::setAdjointsF (EnergyFunctional.cpp:46-86): adHost, adTarget as [h + F t][8][8]"""
    F = len(poses0)
    hat = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])      # noqa: E731
    adH, adT = np.zeros((F * F, 8, 8)), np.zeros((F * F, 8, 8))
    for h in range(F):
        for t in range(F):
            ll = poses0[t] @ np.linalg.inv(poses0[h])
            R, tr = ll[:3, :3], ll[:3, 3]
            Adj = np.zeros((6, 6))
            Adj[:3, :3], Adj[3:, 3:], Adj[:3, 3:] = R, R, hat(tr) @ R
            AH, AT = np.eye(8), np.eye(8)
            AH[:6, :6] = -Adj.T
            a = float(f32(np.exp(affs[t, 0] - affs[h, 0]) * exps[t] / exps[h]))
            AT[6, 6], AH[6, 6], AT[7, 7], AH[7, 7] = -a, a, -1.0, a
            for M in (AH, AT):
                M[6, :] *= 10.0
                M[7, :] *= 1000.0
            adH[h + F * t], adT[h + F * t] = AH, AT
    return adH, adT


def make(seed, F, per_host, prm=None, shift=0, targets_per_point=None, shape=(H, W), K=K):
    H, W = shape
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    # worldToCam of every frame: frame 0 is the world, frame 1 a pure rotation of it, the others small motions
    poses = [_T44(se3((0, 0, 0), (0, 0, 0))), _T44(se3((0.006, -0.004, 0.01), (0, 0, 0)))]
    for f in range(2, F):
        poses.append(_T44(se3(0.012 * rng.standard_normal(3), 0.03 * rng.standard_normal(3))))
    poses0 = [T @ _T44(se3(0.0005 * rng.standard_normal(3), 0.001 * rng.standard_normal(3) * (f > 1))) for f, T in enumerate(poses)]
    affs = np.stack([0.02 * rng.standard_normal(F), 2.0 * rng.standard_normal(F)], axis=1)
    exps = rng.uniform(0.8, 1.25, F)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    images = []
    for f in range(F):
        T = poses[f]
        Hom = Km @ (T[:3, :3] + np.outer(T[:3, 3], PLANE_N) / PLANE_D) @ np.linalg.inv(Km)
        back = np.linalg.inv(Hom) @ np.stack([xx.ravel(), yy.ravel(), np.ones(H * W)])
        img = texture(back[0] / back[2], back[1] / back[2]).reshape(H, W)
        images.append(np.exp(affs[f, 0]) * img * exps[f] / exps[0] + affs[f, 1])
    images = np.stack(images).astype(f32)
    host, uv, ids = [], [], []
    for h, cnt in enumerate(per_host):
        u = rng.integers(3, W - 3, cnt).astype(np.float64)
        v = rng.integers(3, H - 3, cnt).astype(np.float64)
        if cnt >= 40:                                                # on and beyond the border, beside the NaN patch, inside the flat part
            u[:5], v[:5] = [W - 4, W - 2.5, 13.0, 52.0, 1.0], [20.0, 22.0, 32.0, 6.0, 9.0]
        T = poses[h]
        n_h = T[:3, :3] @ PLANE_N
        d_h = PLANE_D + n_h @ T[:3, 3]
        idp = (n_h[0] * (u - cx) / fx + n_h[1] * (v - cy) / fy + n_h[2]) / d_h
        host += [h] * cnt
        uv.append(np.stack([u, v], axis=1))
        ids.append(idp * (1.0 + 0.03 * rng.standard_normal(cnt)))
    host, uv, ids = np.array(host, np.int32), np.concatenate(uv).astype(f32), np.concatenate(ids).astype(f32)
    n = len(host)
    idz = (ids * (1.0 + 0.01 * rng.standard_normal(n))).astype(f32)
    if n >= 8:
        idz[5], idz[6] = 1e4, -1e4                                   # one of the two turns 1 / ptp[2] negative for every target with t_z != 0
    color, weights = np.zeros((n, 8), f32), np.zeros((n, 8), f32)
    for i in range(n):
        img = images[host[i]]
        for k, (px, py) in enumerate(PATTERN):
            x, y = int(min(max(uv[i, 0] + px, 1), W - 2)), int(min(max(uv[i, 1] + py, 1), H - 2))
            gx, gy = 0.5 * (img[y, x + 1] - img[y, x - 1]), 0.5 * (img[y + 1, x] - img[y - 1, x])
            color[i, k] = img[y, x]
            weights[i, k] = np.sqrt(2500.0 / (2500.0 + np.nan_to_num(gx * gx + gy * gy)))
    bright = rng.random(n) < 0.12                                    # a brightness error: the second Huber branch, OUTLIER by energy
    color[bright] += f32(60.0)
    dim = ~bright & (rng.random(n) < 0.15)
    color[dim] += f32(11.0)                                          # |r| > huberTH, yet inside the energy threshold
    color = np.where(np.isfinite(color), color, f32(100.0)).astype(f32)
    point, target = [], []
    empty_pair = (F - 1, 0)                                          # no residual of this (host, target) pair
    for i in range(n):
        cand = [t for t in range(F) if t != host[i] and (host[i], t) != empty_pair]
        if i % 9 == 4 and host[i] == 0:
            cand = [1]                                               # towards the pure rotation only: Hdd_accAF is 0, H clamps at 1e-10
        elif targets_per_point is not None and len(cand) > targets_per_point and i % 3:
            cand = sorted(rng.choice(cand, targets_per_point, replace=False).tolist())
        point += [i] * len(cand)
        target += cand
    point, target = np.array(point, np.int32), np.array(target, np.int32)
    m = len(point)
    state = np.zeros(m, np.int32)
    energy = rng.uniform(0.0, 900.0, m).astype(f32)
    oob = rng.random(m) < 0.04
    if m > 1:
        oob[1] = True
    state[oob] = 1
    state[~oob & (rng.random(m) < 0.05)] = 2
    precalc = np.zeros((F * F, 27), f32)
    for h in range(F):
        for t in range(F):
            precalc[h * F + t] = _precalc(Km, poses[h], poses[t], poses0[h], poses0[t], affs[h], affs[t], exps[h], exps[t])
    c = types.SimpleNamespace(H=H, W=W, F=F, K=tuple(np.float32(K).tolist()), prm=dict(prm or {}), images=images, host=host, uv=uv, color=color,
                              weights=weights, ids=ids, idz=idz, ids2=(ids * (1.0 + 0.02 * rng.standard_normal(n))).astype(f32), point=point,
                              target=target, state=state, energy=energy, precalc=precalc,
                              th=(ENERGY_TH * rng.uniform(0.8, 1.2, F)).astype(f32), prior=rng.uniform(0.0, 50.0, n).astype(f32) * (rng.random(n) < 0.5),
                              delta=(0.01 * rng.standard_normal(n)).astype(f32), lf=np.zeros((n, 6), f32), shift=shift, poses=poses, poses0=poses0,
                              affs=affs, exps=exps)
    c.prior = c.prior.astype(f32)
    c.adH, c.adT = _adjoints(poses0, affs, exps)
    if shift:
        c.lf = (rng.uniform(0.0, 5.0, (n, 6)) * (rng.random((n, 1)) < 0.3)).astype(f32)
    if n >= 8:
        clamp = (np.arange(n) % 9 == 4) & (host == 0)
        c.prior[clamp] = 0
        c.lf[clamp] = 0
    return c


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["f2_single"] = make(10, 2, [1, 0])
    c["f3_5"] = make(2, 3, [5, 5, 5], shift=1)
    c["f3_513"] = make(3, 3, [513, 3, 2], prm=dict(affine_opt_mode_a=-1.0, affine_opt_mode_b=-1.0), targets_per_point=1)
    c["f8_1100"] = make(4, 8, [1100] + [40] * 7, shift=1, targets_per_point=4)
    return c
