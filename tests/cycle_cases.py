"""One consistent scene for the multi-cycle tests (tests/cycle_harness.py, tests/test_cycle_oracle.py, tests/test_cycle_gpu.py): a textured
plane at 96 x 128 seen by F = 4 window frames at slightly different poses, four further keyframes K1 .. K4 along a translating path and
two non-keyframe images after every keyframe, on which the immature points are traced.  Every image is rendered from its true pose;
the window's initial points read color[8] / weights[8] from their host image as ImmaturePoint's constructor does and carry the plane's
inverse depth plus a few per cent of noise; adjoints and precalc come from the evaluation poses, which are the true poses plus a small
seeded perturbation; the initial prior is zero but for the first frame's pose prior.  The initial history is what a running system
holds for points that came through makeKeyFrame (the two latest residuals IN, four good residuals): the columns' defaults say OOB, and
flagPointsForRemoval would drop every initial point in the first cycle.  K2 carries a NaN patch and K3 a block of foreign texture, so
residuals towards them go OOB and OUTLIER.

Frames are named by a global index: 0 .. 3 the initial window, 4 .. 7 the keyframes K1 .. K4.  ``frame_inputs(ids)`` gives everything
a caller supplies for a window whose slots hold the frames `ids`; ``reindex(ids, leaving, new)`` is the window after a frame left
and the new keyframe took slot F - 1."""
import functools
import types

import numpy as np

import activate_cases as ac
import immature_cases as ic
import window_cases as wc

f32 = np.float32
H, W, F = 96, 128, 4
K4 = (110.0, 104.0, 66.5, 45.25)                      # winedit_cases.cycle_case()'s camera
CYCLES = 4
LEAVING = (0, F // 2 - 1, F - 2, 0)                   # the slot that leaves in cycle 1 .. 4: the first, a middle one, F - 2, the first again
PER_HOST = 34
IMMATURE_PER_HOST = 70                                # the initial hosts' immature points (the keyframes' come from the selector)
SELECT_DENSITY = 90.0
MIN_ACT_DIST = 2.0
# flagPointsForRemoval's settings: the reference's but for minGoodResForMarg.  Its 4 suits a window of 7 frames; with F = 4 a point has
# at most 3 residuals and so collects at most 3 good ones per optimisation, and a point activated in one cycle could never be
# marginalised with the frame that leaves in the next.
FLAG_PARAMS = dict(min_good_res_for_marg=3)
ENERGY_TH = f32(8 * 12.0 * 12.0)                      # patternNum * setting_outlierTH
# The evaluation poses' perturbation.  Seed and size were chosen on the CPU (the host chain alone) so that over the four cycles at
# least one Gauss-Newton step is accepted and at least one rejected, and the kept points' median inverse-depth error does not grow.
POSE_SEED, POSE_ROT, POSE_TRANS = 5, 4e-4, 4e-4
SCENE_SEED = 83
PRIOR_POSE = np.array([1e10] * 3 + [1e11] * 3)       # setting_initialTransPrior, setting_initialRotPrior: the first frame's
PRIOR_AFF = np.array([1e12, 1e8])                     # setting_affineOptModeA / B
C_PRIOR = np.full(4, 5e9)                             # setting_initialCalibHessian


def T_cw(pose):
    """worldToCam 4 x 4 of a (R_wc, p) pose"""
    R, p = pose
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ p
    return T


def T_wc34(pose):
    """camToWorld 3 x 4"""
    R, p = pose
    return np.concatenate([R, np.asarray(p, np.float64)[:, None]], axis=1)


def plane_idepth(pose, u, v, Z0):
    R, p = pose
    fx, fy, cx, cy = K4
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ R.T
    return d[..., 2] / (Z0 - p[2])


def color_weights(img, uv):
    """color[8] / weights[8] as ImmaturePoint's constructor reads them at integer pixels"""
    n = len(uv)
    color, weights = np.zeros((n, 8), f32), np.zeros((n, 8), f32)
    for i in range(n):
        for k, (px, py) in enumerate(wc.PATTERN):
            x, y = int(uv[i, 0]) + px, int(uv[i, 1]) + py
            gx, gy = f32(0.5) * (img[y, x + 1] - img[y, x - 1]), f32(0.5) * (img[y + 1, x] - img[y - 1, x])
            color[i, k] = img[y, x]
            weights[i, k] = np.sqrt(f32(2500.0) / (f32(2500.0) + (gx * gx + gy * gy)))
    return color, weights


def reindex(ids, leaving, new):
    """the frames in the window's slots after slot `leaving` left (the frames above it move down) and `new` took slot F - 1"""
    return tuple(f for k, f in enumerate(ids) if k != leaving) + (new,)


class Case:
    def frame_inputs(self, ids):
        """what a caller supplies for the window whose slots hold the frames `ids`: precalc [h F + t][27], adH / adT [h + F t][8][8],
        delta, prior, delta_prior, cPrior, cDelta, the frame energy thresholds, and for the activation KRKi1 / Kt1 into the newest
        slot, the 14-float precalc, the camToWorld poses and the newest frame's worldToCam"""
        n = len(ids)
        Km = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
        T = [T_cw(self.eval_poses[f]) for f in ids]
        zero, one = np.zeros(2), 1.0
        pc = np.zeros((n * n, 27), f32)
        for h in range(n):
            for t in range(n):
                pc[h * n + t] = wc._precalc(Km, T[h], T[t], T[h], T[t], zero, zero, one, one)
        adH, adT = wc._adjoints(T, np.zeros((n, 2)), np.ones(n))
        poses = [self.eval_poses[f] for f in ids]
        K1, Kt1 = np.zeros((n, 3, 3), f32), np.zeros((n, 3), f32)
        for h in range(n):
            K1[h], Kt1[h] = ac.distance_precalc(K4, *ac.relative(poses, h, n - 1))
        prior = np.zeros((n, 8))
        for k, f in enumerate(ids):
            prior[k, 6:] = PRIOR_AFF                  # the first frame's pose prior is in the initial HM
        return types.SimpleNamespace(F=n, ids=tuple(ids), precalc=pc, adH=adH, adT=adT, delta=np.zeros((n, 8)), prior=prior, delta_prior=np.zeros((n, 8)),
                                     cPrior=C_PRIOR.copy(), cDelta=np.zeros(4), th=np.full(n, ENERGY_TH, f32), KRKi1=K1, Kt1=Kt1,
                                     pre14=ac.precalc(poses, (0.0, 0.0)), T_w_c=np.stack([T_wc34(p) for p in poses]), T_kf_w=T[n - 1][:3],
                                     images=np.stack([self.images[f] for f in ids]))

    def trace_inputs(self, ids, cycle, j):
        """hostToFrame_KRKi, Kt and the affine pair of every slot's frame into the cycle's j-th in-between image"""
        Rt, pt = self.trace_poses[cycle][j]
        out = [ic.precalc32(K4, Rt.T @ self.eval_poses[f][0], Rt.T @ (self.eval_poses[f][1] - pt)) for f in ids]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])

    def idepth_error(self, ids, host, uv, idepth):
        """the relative error of window points' inverse depths against the plane's, per point (true poses)"""
        want = np.array([plane_idepth(self.poses[ids[h]], np.float64(u), np.float64(v), self.Z0) for h, (u, v) in zip(host, uv)])
        return np.abs(np.asarray(idepth, np.float64) - want) / want


@functools.lru_cache(maxsize=None)
def case():
    sc = ic.Scene(SCENE_SEED, H, W, K4)
    rng = sc.rng
    c = Case()
    c.H, c.W, c.F, c.K4, c.Z0 = H, W, F, K4, sc.Z0
    path = np.array([0.08, 0.015, 0.004])
    c.poses, c.images, c.trace_poses, c.trace_images = [], [], [], []
    for f in range(F):                                # the initial window: slightly different poses around the origin
        c.poses.append((ic.rot(*rng.uniform(-0.012, 0.012, 2), rng.uniform(-0.03, 0.03)), np.append(rng.uniform(-0.1, 0.1, 2), rng.uniform(-0.02, 0.02))))
    for k in range(1, CYCLES + 1):                    # K1 .. K4 along the path, two in-between images after each
        c.poses.append((ic.rot(*rng.uniform(-0.01, 0.01, 2), rng.uniform(-0.02, 0.02)), path * k + rng.uniform(-0.006, 0.006, 3)))
        c.trace_poses.append([(ic.rot(*rng.uniform(-0.008, 0.008, 2), rng.uniform(-0.02, 0.02)), path * (k + (j + 1) / 3.0)) for j in range(2)])
    c.images = [sc.render(R, p) for R, p in c.poses]
    c.trace_images = [[sc.render(R, p) for R, p in pair] for pair in c.trace_poses]
    yy, xx = np.mgrid[0:H, 0:W]
    # the disturbances sit in keyframes that later cycles linearize residuals towards (K4's are only created, in the last step)
    c.images[F + 1][H // 5:H // 5 + 12, W // 6:W // 6 + 16] = np.nan                                  # K2: a NaN patch
    y0, x0 = H // 3, W // 3
    c.images[F + 2][y0:y0 + 30, x0:x0 + 40] = (128 + 100 * np.sin(2.1 * xx) * np.cos(1.7 * yy))[y0:y0 + 30, x0:x0 + 40].astype(f32)   # K3: foreign texture
    prng = np.random.default_rng(POSE_SEED)
    c.eval_poses = [(ic.rot(*(POSE_ROT * prng.standard_normal(3))) @ R, p + POSE_TRANS * prng.standard_normal(3)) for R, p in c.poses]
    # the window's initial points and residuals: every point sees every other frame
    host = np.repeat(np.arange(F, dtype=np.int32), PER_HOST)
    n = len(host)
    uv = np.stack([rng.integers(8, W - 8, n), rng.integers(8, H - 8, n)], axis=1).astype(f32)
    truth = np.array([plane_idepth(c.poses[h], np.float64(u), np.float64(v), c.Z0) for h, (u, v) in zip(host, uv)])
    ids = (truth * (1.0 + 0.05 * rng.standard_normal(n))).astype(f32)
    color, weights = np.zeros((n, 8), f32), np.zeros((n, 8), f32)
    for h in range(F):
        color[host == h], weights[host == h] = color_weights(c.images[h], uv[host == h])
    point = np.repeat(np.arange(n, dtype=np.int32), F - 1)
    target = np.array([t for h in host for t in range(F) if t != h], np.int32)
    c.win = types.SimpleNamespace(host=host, uv=uv, color=color, weights=weights, ids=ids, idz=ids.copy(), point=point, target=target,
                                  state=np.zeros(len(point), np.int32), energy=np.zeros(len(point), f32))
    c.priorF, c.deltaF = np.zeros(n, f32), np.zeros(n, f32)
    # every third point names its two oldest targets, the older one second, instead of the two latest (any target is a valid entry):
    # only so does the frame removal of cycle 2 find targets below the leaving slot, which stay, beside those it lowers and clears
    latest = np.array([[t for t in range(F - 1, -1, -1) if t != h][-2 if i % 3 == 0 else 0:][:2] for i, h in enumerate(host)], np.int32)
    c.history = dict(num_good=np.full(n, 4, np.int32), max_rel_baseline=np.zeros(n, f32), last_target=latest, last_state=np.zeros((n, 2), np.int32),
                     is_new=np.ones(len(point), np.int32))
    c.initial_error = float(np.median(c.idepth_error(tuple(range(F)), host, uv, ids)))
    # the initial hosts' immature points: integer pixels away from the border, every selector type
    c.immature = [dict(uv=np.stack([rng.integers(6, W - 6, IMMATURE_PER_HOST), rng.integers(6, H - 6, IMMATURE_PER_HOST)], axis=1).astype(np.int32),
                       type=rng.choice([1.0, 2.0, 4.0], IMMATURE_PER_HOST).astype(f32)) for _ in range(F)]
    N = 4 + 8 * F
    c.HM, c.bM = np.zeros((N, N)), np.zeros(N)
    c.HM[4:10, 4:10] = np.diag(PRIOR_POSE)            # the reference's prior on the first frame's pose
    c.ids0 = tuple(range(F))
    c.new_frame = tuple(F + k for k in range(CYCLES))
    return c


# What the host chain measured over the four cycles (tests/test_cycle_oracle.py asserts them): the most points and residuals the
# window ever held, the most immature points one host ever held.  tests/test_cycle_gpu.py opens its handles with exactly these.
PEAK_POINTS, PEAK_RESIDUALS, PEAK_IMMATURE = 140, 414, 93
