"""Cameras that are NOT symmetric under an exchange of the image axes, for the tracker core: fx != fy, a principal point off the centre,
portrait as well as landscape frames, keyframe pixels off the grid and on / just outside the frame border.  synth.make_alignment and
tests/subpixel_cases.py take their camera from synth.intrinsics (fx == fy, centred), under which fx-for-fy, cx-for-cy and W-for-H slips
are invisible.  Pure numpy: the same bytes here and on the GPU box."""
import importlib

import numpy as np

import subpixel_cases as sc


def _tall(H, W):
    fx = 0.78125 * W
    return fx, 0.8 * fx, 0.41 * W + 0.3, 0.56 * H - 0.2


def _wide(H, W):
    fx = 0.78125 * W
    return fx, 1.25 * fx, 0.58 * W - 0.4, 0.43 * H + 0.1


def _davis(H, W):
    """the DAVIS240C calibration of the reference's datasets (199.09 / 198.83, principal point 132.19 / 110.71 at 240 x 180), scaled to the
    frame.  Its anisotropy is 1.3e-3: a parity case, too weak to tell fx from fy at the suite's tolerances"""
    fx = 0.78125 * W
    return fx, fx * 198.83 / 199.09, 132.19 * W / 240.0, 110.71 * H / 180.0


CAMERAS = {"tall": _tall, "wide": _wide, "davis": _davis}
DISCRIMINATING = ("tall", "wide")                           # davis is exempt from the discriminating-power condition
FRAMES = [(61, 83), (83, 61), (120, 160), (160, 120)]       # H x W; (240, 320) / (320, 240) only where a kernel needs > 2 048 points
PORTRAIT, LANDSCAPE, BIG_PORTRAIT = (83, 61), (61, 83), (320, 240)

# a generic start, as in tests/test_instances_gpu.py: at the identity integer keyframe pixels project onto pixel centres, where the bilinear
# gradient is discontinuous
PS = np.array([1e-3, -2e-3, 5e-4])


def QS():
    synth = importlib.import_module("slam-eds_amd.synth")
    return synth.quat_from_axis_angle([0.3, -0.5, 0.8], 2e-3)


def eval_pose(seed=3, ang=0.003, t=0.002):
    """the evaluation pose of the row tests (tests/test_parity_gpu.py's)"""
    synth = importlib.import_module("slam-eds_amd.synth")
    rng = np.random.default_rng(seed)
    return t * rng.standard_normal(3), synth.quat_from_axis_angle(rng.standard_normal(3), ang)


# a pose that throws 20 - 85 % of the points of a portrait frame outside it (asserted where it is used)
P_OUT = np.array([0.25, -0.15, 0.02])


def Q_OUT():
    synth = importlib.import_module("slam-eds_amd.synth")
    return synth.quat_from_axis_angle([0.1, 1.0, -0.2], 0.04)


def EDGE_PIXELS(H, W):
    """the last row / column and pixels with x or y in (-1, 0) (negative cell: sign extension of the packed column), pixels ON row 0 and
    column 0 (negative at pyramid levels >= 1 through (u + 0.5) / 2^l - 0.5) and three pixels 1e-13 below an integer (cell k - 1, the fp32
    fraction rounds to 1.0f)"""
    pts = sc.LAST(H, W) + sc.JUST_OUTSIDE(H, W)
    pts += [(0.0, 0.0), (0.0, 7.0), (0.0, H - 1.0), (0.0, H / 2.0 + 0.25), (5.0, 0.0), (W - 1.0, 0.0), (W / 2.0 + 0.75, 0.0)]
    pts += [(20.0 - 1e-13, 4.0), (9.0, 5.0 - 1e-13), (17.0 - 1e-13, 3.0 - 1e-13)]
    return pts


def camera(name_or_fn, H, W):
    return (CAMERAS[name_or_fn] if isinstance(name_or_fn, str) else name_or_fn)(H, W)


def camera_alignment(seed, H, W, N, camera_name, pixels="integer", extra=(), margin=2, **kw):
    """synth.make_alignment(seed, H, W, N, margin=margin, **kw)'s points (same raster order of the 20 x 20 cells, gradients, inverse depths,
    weights, ground truth), optionally a uniform [0, 1) offset on every pixel, then the pixels of `extra` verbatim (random gradients,
    inverse depths and weights of their own); norm_coord = (px - c) / f and the frame (synth.render_frame at the ground truth) under the
    case's camera.  The Alignment carries that camera."""
    synth = importlib.import_module("slam-eds_amd.synth")
    base = synth.make_alignment(seed, H=H, W=W, N=N, margin=margin, **kw)
    rng = np.random.default_rng([int(seed), 0x1C])
    px = base.coord.copy()
    if pixels == "subpixel":
        px = px + rng.uniform(0.0, 1.0, size=px.shape)
    elif pixels != "integer":
        raise ValueError(f"pixels must be 'integer' or 'subpixel', not {pixels!r}")
    grad, idp, w = base.grad, base.idp, base.weights
    ex = np.asarray(extra, dtype=np.float64).reshape(-1, 2)
    if len(ex):
        px = np.vstack([px, ex])
        grad = np.vstack([grad, rng.standard_normal((len(ex), 2))])
        idp = np.concatenate([idp, rng.uniform(0.2, 1.0, size=len(ex))])
        w = np.concatenate([w, np.ones(len(ex)) if kw.get("unit_weights") else 1.0 - rng.uniform(0.0, 0.3, size=len(ex))])
    fx, fy, cx, cy = camera(camera_name, H, W)
    norm = np.column_stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy])
    frame = synth.render_frame(H, W, (fx, fy, cx, cy), norm, grad, idp, base.p_true, base.q_true, base.v_true,
                               blur_ksize=kw.get("blur_ksize", 7), blur_sigma=kw.get("blur_sigma", 1.5), noise=kw.get("noise", 0.05), rng=rng)
    return synth.Alignment(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, norm_coord=np.ascontiguousarray(norm), grad=np.ascontiguousarray(grad),
                           idp=np.ascontiguousarray(idp), weights=np.ascontiguousarray(w), frame=np.ascontiguousarray(frame), coord=px,
                           p_true=base.p_true, q_true=base.q_true, v_true=base.v_true, p0=base.p0, q0=base.q0, v0=base.v0)


def replace(al, **kw):
    return type(al)(**{**al.__dict__, **kw})


def isotropic(al):
    """the same norm_coord seen through fy := fx: what a kernel that scales the row displacement with fx computes"""
    return replace(al, fy=al.fx)


_cache = {}


def row_alignment(cam, H, W):
    """the alignment of the row tests: 300 sub-pixel points plus EDGE_PIXELS"""
    key = ("row", cam, H, W)
    if key not in _cache:
        _cache[key] = camera_alignment(ROW_SEED + 7 * H + W, H, W, 300, cam, pixels="subpixel", extra=EDGE_PIXELS(H, W))
    return _cache[key]


ROW_SEED = 4100
ROW_CASES = [(cam, H, W) for cam in DISCRIMINATING for (H, W) in FRAMES]


# -- solve cases: batches of three alignments on a portrait frame, 8 iterations from (PS, QS)
SOLVE_ITERS = 8
SOLVE_B = 3
SOLVE_TAU = 0.004                                          # per-point Huber threshold of the Huber instantiations
# the ground-truth offset of the solve cases: three times make_alignment's default, so that LM has rejected steps on the way
SOLVE_KW = dict(rot_deg=0.6, trans_norm=0.012)
# The frame of a point count.  (83, 61) holds 4 503 distinct pixels inside the margin, so every count up to 2 048 fits; but the oracle's
# pose-only solve rejects no step there once a fifth of the pixels carry a point (N = 1 011 with the Huber weights, N = 2 011 always:
# 30 seeds, three start distances, lambda0 1e-2 .. 1e-4 tried), and a solve without a rejected step does not exercise the kernels'
# restore path.  Those counts therefore sit on the next portrait frames.  The REF12 solve does reject at (83, 61) with 2 000 points.
SOLVE_FRAMES = {499: (83, 61), 1011: (160, 120), 2011: (320, 240), 4059: (320, 240),
                2000: (83, 61), 1989: (83, 61), 3989: (320, 240), 9000: (320, 240)}
# Seeds per case, chosen on the CPU with the oracle alone: each alignment's solve rejects at least one step and accepts at least two
# (tests/test_intrinsics_oracle.py asserts it).  lm6: (N, sampler, Huber); ref12: (N, sampler, NC), the cap of 8 iterations reached.
# ("ref12", 2000, 0, 1) is the exception: the bicubic NC solve rejected no step for any of 300 seeds, three loss settings and 1 / 2 / 5
# blocks, so its seeds only guarantee accepted steps and an exit on the cap.
SOLVE_SEEDS = {
    ("lm6", 499, 0, 0): (7000, 7001, 7002), ("lm6", 499, 1, 0): (7000, 7001, 7002),
    ("lm6", 1011, 0, 0): (7000, 7001, 7002), ("lm6", 1011, 0, 1): (7001, 7003, 7006),
    ("lm6", 1011, 1, 0): (7000, 7001, 7002), ("lm6", 1011, 1, 1): (7001, 7002, 7003),
    ("lm6", 2011, 0, 0): (7000, 7001, 7002), ("lm6", 2011, 0, 1): (7001, 7002, 7005),
    ("lm6", 2011, 1, 0): (7000, 7001, 7002), ("lm6", 2011, 1, 1): (7000, 7001, 7002),
    ("lm6", 4059, 0, 0): (7000, 7001, 7002), ("lm6", 4059, 0, 1): (7001, 7009, 7011),
    ("lm6", 4059, 1, 0): (7000, 7001, 7002), ("lm6", 4059, 1, 1): (7001, 7002, 7004),
    ("ref12", 2000, 0, 0): (7101, 7105, 7108), ("ref12", 2000, 0, 1): (7100, 7103, 7104),
    ("ref12", 2000, 1, 0): (7100, 7101, 7102), ("ref12", 2000, 1, 1): (7101, 7104, 7105),
    ("ref12", 1989, 0, 0): (7102, 7107, 7114), ("ref12", 1989, 1, 0): (7100, 7101, 7102),
    ("ref12", 3989, 0, 0): (7100, 7101, 7102), ("ref12", 3989, 1, 0): (7100, 7101, 7102),
    ("ref12", 9000, 0, 0): (7100, 7101, 7102), ("ref12", 9000, 1, 0): (7100, 7101, 7102),
}
NO_REJECTED_STEP = {("ref12", 2000, 0, 1)}
REF12_KW = dict(num_blocks=2, loss_param=0.3)              # with the Huber loss; every family below holds two residual blocks

# The code families of the persistent kernels: the first instantiation of every distinct (S, Q, K > 1, G > 1) of eds_fused6_kernel, of
# every (S, NC, Q, K > 1) of eds_fused12_kernel, and the candidate-group list.  Kept as a literal so that the GPU test has one id per
# family; the GPU test asserts that the library's own lists give exactly these.
FUSED6_FAMILIES = [(S, Q, K, G) for S, Q, K, G in (
    (0, 4, 0, 0), (0, 3, 0, 0), (1, 4, 0, 0), (1, 3, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (0, 2, 0, 0), (1, 4, 1, 0), (1, 3, 1, 0), (0, 4, 1, 0),
    (0, 3, 1, 0), (0, 2, 1, 0), (0, 1, 1, 0), (0, 0, 1, 0), (1, 0, 0, 0), (1, 0, 1, 0), (0, 0, 1, 1), (0, 1, 1, 1), (0, 3, 1, 1), (0, 2, 1, 1),
    (0, 4, 1, 1), (1, 3, 1, 1), (1, 4, 1, 1), (1, 0, 1, 1))]
FUSED12_FAMILIES = [(0, 0, 0, 1), (1, 0, 0, 1), (0, 0, 2, 1), (0, 0, 1, 1), (0, 0, 2, 0), (0, 0, 1, 0), (0, 1, 1, 0), (0, 0, 0, 0), (0, 1, 0, 0),
                    (1, 0, 0, 0), (1, 1, 0, 0)]
FUSED12_GROUPS = [(0, 512, 0, 8, 0, 2), (0, 512, 0, 8, 0, 4), (1, 512, 0, 8, 0, 2), (1, 512, 0, 8, 0, 4), (0, 512, 0, 4, 0, 2), (1, 512, 0, 4, 0, 2),
                  (0, 512, 0, 4, 0, 4), (1, 512, 0, 4, 0, 4)]


def fused6_family(inst):
    S, P, T, Q, K, G = inst
    return (S, Q, int(K > 1), int(G > 1))


def fused12_family(inst):
    S, T, CAP, NC, K, Q = inst
    return (S, NC, Q, int(K > 1))


def first_of_each(instances, family):
    out = {}
    for inst in instances:
        out.setdefault(family(inst), inst)
    return out


def fused6_points(inst):
    """the point count tests/test_instances_gpu.py gives an instantiation: a little under its lane slots"""
    S, P, T, Q, K, G = inst
    cap = P * (512 if K > 1 else T) * K if P > 0 else 2500
    return cap - 37 if K > 1 else min(cap - 13, 2000)


def fused12_points(K, G):
    return (2000 if K <= 4 else (4000 if K == 8 else 9000)) if G == 1 else 500 * K - 11


def solve_frame(N):
    return SOLVE_FRAMES[N]


def solve_alignment(seed, N, cam="tall"):
    """one alignment of a solve case: sub-pixel points and EDGE_PIXELS under `cam` on solve_frame(N), the frame rounded to fp32 (what the
    library stores, so that the oracle sees the same frame)"""
    H, W = solve_frame(N)
    key = ("solve", cam, seed, N)
    if key not in _cache:
        ex = EDGE_PIXELS(H, W)
        _cache[key] = f32_frame(camera_alignment(seed, H, W, N - len(ex), cam, pixels="subpixel", extra=ex, **SOLVE_KW))
    return _cache[key]


def solve_case(key, cam="tall"):
    return [solve_alignment(s, key[1], cam) for s in SOLVE_SEEDS[key]]


def f32_frame(al):
    """the alignment with its frame rounded to fp32, as the library stores it"""
    return replace(al, frame=np.ascontiguousarray(al.frame, dtype=np.float32).astype(np.float64))


# -- point maintenance: the pose of tests/test_points_gpu.py and two points whose fate changes under a rows / cols exchange
P_PTS = np.array([0.06, -0.03, 0.01])


def Q_PTS():
    synth = importlib.import_module("slam-eds_amd.synth")
    return synth.quat_from_axis_angle([0.1, 1.0, 0.2], 0.05)


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def exchange_targets(H, W):
    """two projections (xp, yp) between min(H, W) and max(H, W) along one axis and well inside along the other.  Tracker::getCoord erases
    xp > cols and yp > rows: on a portrait frame (rows > cols) the first is erased and the second kept, on a landscape one the other
    way round, and an exchange of rows and cols flips both"""
    lo, hi = min(H, W), max(H, W)
    mid = 0.5 * (lo + hi)
    return [(mid, 0.4 * lo), (0.3 * lo, mid)]


def points_alignment(seed, H, W, N, cam, p=None, q=None):
    """N - 2 sub-pixel points (margin 2) and, last, the two points that project onto exchange_targets(H, W) under the pose (p, q)"""
    p = P_PTS if p is None else p
    q = Q_PTS() if q is None else q
    al = camera_alignment(seed, H, W, N - 2, cam, pixels="subpixel")
    fx, fy, cx, cy = al.fx, al.fy, al.cx, al.cy
    R = _quat_to_R(q)
    norm, idp, px = [], [], []
    for k, (xp, yp) in enumerate(exchange_targets(H, W)):
        depth = 1.7 + 0.6 * k
        P = depth * np.array([(xp - cx) / fx, (yp - cy) / fy, 1.0])
        X = R.T @ (P - p)
        norm.append((X[0] / X[2], X[1] / X[2]))
        idp.append(1.0 / X[2])
        px.append((fx * norm[-1][0] + cx, fy * norm[-1][1] + cy))
    rng = np.random.default_rng([int(seed), 0x2D])
    return replace(al, norm_coord=np.ascontiguousarray(np.vstack([al.norm_coord, norm])), idp=np.concatenate([al.idp, idp]),
                   coord=np.vstack([al.coord, px]), grad=np.ascontiguousarray(np.vstack([al.grad, rng.standard_normal((2, 2))])),
                   weights=np.concatenate([al.weights, [0.9, 0.8]]))


def get_coord_longdouble(norm_coord, idp, coord, K, rows, cols, p, q):
    """Tracker::getCoord(true) (Tracker.cpp:343-372) written out once more, in np.longdouble and point by point"""
    ld = np.longdouble
    fx, fy, cx, cy = (ld(k) for k in K)
    R = _quat_to_R(np.asarray(q, dtype=ld))
    kept, new = [], []
    for i in range(len(idp)):
        z = ld(1) / ld(idp[i])
        P = R @ np.array([ld(norm_coord[i, 0]) * z, ld(norm_coord[i, 1]) * z, z], dtype=ld) + np.asarray(p, dtype=ld)
        xp, yp = fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy
        if not (xp < 0 or xp > cols or yp < 0 or yp > rows):
            kept.append(i)
            new.append((xp, yp))
    new = np.array(new, dtype=ld).reshape(-1, 2)
    tracks = new - np.asarray(coord, dtype=ld)[kept]
    return dict(kept=np.array(kept, dtype=np.int64), coord=new, tracks=tracks, mean_sq_flow=(tracks ** 2).sum() / max(len(kept), 1))


def residual_row_displacement_with_fx(al, p, q, v, sampling="bicubic"):
    """the plain one-block residual with the projection in the library's displacement form, u = u0 + fx (Px / Pz - x0),
    v = v0 + f (Py / Pz - y0), and the slip under test in it: f = fx where fy belongs (csrc/eds_device.hpp project_point)"""
    import np_oracle as npo
    _, P, _, _ = npo.project(al, p, q)
    x0, y0 = al.norm_coord[:, 0], al.norm_coord[:, 1]
    u = (al.fx * x0 + al.cx) + al.fx * (P[:, 0] / P[:, 2] - x0)
    vv = (al.fy * y0 + al.cy) + al.fx * (P[:, 1] / P[:, 2] - y0)
    m = npo.flow_matrix(al) @ np.asarray(v)
    E = (npo.bicubic if sampling == "bicubic" else npo.bilinear)(al.frame, vv, u)[0]
    return al.weights * (m / np.sqrt(npo.S0 + np.sum(m * m)) - E)


# -- the pyramid case: 3 levels from (160, 120) under `tall`; level l takes the first PYR_COUNTS[l] points, so the pixels on row 0 and
# column 0 (negative at levels >= 1: (0 + 0.5) / 2^l - 0.5) come first
PYR_H, PYR_W, PYR_COUNTS = 160, 120, [1200, 600, 300]
PYR_KW = dict(rot_deg=0.6, trans_norm=0.012, blur_ksize=9, blur_sigma=2.5)          # tests/test_pyramid.py's batched case
PYR_ITERS = [6, 6, 6]
# seeds whose LM6 and REF12 oracle tracks end nearer the truth than they start (with 300 points on 40 x 30 pixels the coarse levels
# reject nearly every step, under the symmetric camera as well, and one seed in three does not get nearer)
PYR_SEEDS = (3300, 3302, 3304)
PYR_REF12_KW = dict(num_blocks=4, loss_param=0.3)                                   # with the Huber loss


def pyramid_alignment(seed=3300, cam="tall"):
    key = ("pyr", cam, seed)
    if key not in _cache:
        H, W = PYR_H, PYR_W
        ex = [(0.0, 0.0), (0.0, 31.0), (0.0, H - 1.0), (0.0, H / 2.0 + 0.25), (44.0, 0.0), (W - 1.0, 0.0), (W / 2.0 + 0.75, 0.0), (0.6, 0.3)]
        al = camera_alignment(seed, H, W, PYR_COUNTS[0] - len(ex), cam, pixels="subpixel", extra=ex, **PYR_KW)
        order = np.concatenate([np.arange(al.N - len(ex), al.N), np.arange(al.N - len(ex))])
        _cache[key] = replace(al, **{k: np.ascontiguousarray(getattr(al, k)[order]) for k in ("norm_coord", "grad", "idp", "weights", "coord")})
    return _cache[key]
