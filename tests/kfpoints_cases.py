"""Cases of the keyframe point-set tests (include/eds_hip_kfpoints.h): refine, clean and projection inputs, shared by the CPU test that
asserts on the oracle alone that they discriminate (tests/test_kfpoints_oracle.py) and the GPU test (tests/test_kfpoints_gpu.py).
Pure numpy: the same bytes here and on the GPU box."""
import importlib

import numpy as np

import intrinsics_cases as ic
import np_kfpoints_oracle as kp
import subpixel_cases as sc

# -- refine ------------------------------------------------------------------------------------------------------------------------
RADII = (0, 3, 11, 15)
BORDERS = [(kp.BORDER_CONSTANT, 255), (kp.BORDER_REPLICATE, 0), (kp.BORDER_REFLECT, 0), (kp.BORDER_REFLECT_101, 0)]
FRAMES = sc.FRAMES                      # 61 x 83, 37 x 45, 9 x 70 (a 23-row window is taller than the frame: reflection repeats), 120 x 160
REFINE_N = 120
AMP_MIN, EVENT_DIFF = 0.5, 0.25         # every spike has |amplitude| >= AMP_MIN: a window's range is 0, >= AMP_MIN, or ~255 at a CONSTANT border
# frame seeds per (H, W, r), found on the oracle alone: every discrimination condition of tests/test_kfpoints_oracle.py holds
REFINE_SEEDS = {(9, 70, 11): 1, (9, 70, 15): 1}         # every other (H, W, r): 0


def refine_points(H, W):
    """REFINE_N sub-pixel points, then SEAMS, LAST, JUST_OUTSIDE and EXACT verbatim; returns (alignment, index ranges of the groups)"""
    groups = [("seams", sc.SEAMS(H, W)), ("last", sc.LAST(H, W)), ("outside", sc.JUST_OUTSIDE(H, W)), ("exact", sc.EXACT)]
    extra = [p for _, g in groups for p in g]
    al = sc.subpixel_alignment(5000 + 7 * H + W, H, W, REFINE_N, extra=extra)
    idx, o = {}, REFINE_N
    for name, g in groups:
        idx[name] = np.arange(o, o + len(g))
        o += len(g)
    return al, idx


def floor_centres(al):
    """the mutation the truncation is told from: the floor of the ORIGINAL pixel (the slot's cell), not the truncated cell + fraction"""
    c = np.floor(np.asarray(al.coord, dtype=np.float64)).astype(np.int64)
    return c[:, 0], c[:, 1]


def _touched(H, W, cx, cy, r):
    """the frame pixels the (2r+1)^2 window at (cx, cy) reads under REFLECT_101, as a mask"""
    k = np.arange(-r, r + 1)
    m = np.zeros((H, W), bool)
    m[np.ix_(kp.border_index(cy + k, H, kp.BORDER_REFLECT_101), kp.border_index(cx + k, W, kp.BORDER_REFLECT_101))] = True
    return m


def refine_frame(H, W, r, seed):
    """a sparse frame: isolated one-pixel spikes of amplitude +-[AMP_MIN, 1] at a density that leaves about half of the (2r+1)^2 windows
    empty; then, for one keyframe pixel with x in (-1, 0) and one 1e-13 below an integer, the windows at the truncated and at the floored
    pixel are cleared and one spike is put where only one of the two windows reads it"""
    al, idx = refine_points(H, W)
    rng = np.random.default_rng([seed, H, W, r])
    area = min(2 * r + 1, H) * min(2 * r + 1, W)
    n = max(2, int(round(np.log(2.0) * H * W / area)))
    f = np.zeros((H, W))
    where = rng.choice(H * W, size=min(n, H * W), replace=False)
    f.ravel()[where] = rng.uniform(AMP_MIN, 1.0, size=len(where)) * rng.choice([-1.0, 1.0], size=len(where))
    if r == 0:
        return f
    tx, ty = kp.truncated(kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy))
    fx_, fy_ = floor_centres(al)
    locked = np.zeros((H, W), bool)
    for group, want in (("outside", lambda p: -1 < p[0] < 0 and p[1] > 0), ("exact", lambda p: p[0] != round(p[0]) or p[1] != round(p[1]))):
        for i in idx[group]:
            if not want(al.coord[i]) or (tx[i], ty[i]) == (fx_[i], fy_[i]):
                continue
            a, b = _touched(H, W, tx[i], ty[i], r), _touched(H, W, fx_[i], fy_[i], r)
            only = np.argwhere((a ^ b) & ~locked)
            if len(only) == 0 or ((a | b) & locked).any():
                continue
            f[a | b] = 0.0
            y, x = only[len(only) // 2]
            f[y, x] = 0.75
            locked |= a | b
            break
    return f


def stored(frame):
    """the frame as a slot stores it and eds_trk_get_event_frame returns it: fp32"""
    return np.asarray(frame, dtype=np.float64).astype(np.float32).astype(np.float64)


def refine_conditions(H, W, r, seed):
    """the discrimination conditions of one (frame, radius) on the oracle alone: dict of the measured figures"""
    al, idx = refine_points(H, W)
    f = stored(refine_frame(H, W, r, seed))
    kpix = kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
    keep = kp.refine(f, kpix, EVENT_DIFF, r, kp.BORDER_REFLECT_101, 0)[1]
    keep_r1 = kp.refine(f, kpix, EVENT_DIFF, r - 1, kp.BORDER_REFLECT_101, 0)[1]
    keep_c = kp.refine(f, kpix, EVENT_DIFF, r, kp.BORDER_CONSTANT, 255)[1]
    keep_fl = kp.refine(f, kpix, EVENT_DIFF, r, kp.BORDER_REFLECT_101, 0, centres=floor_centres(al))[1]
    neg = [i for i in idx["outside"] if -1 < al.coord[i, 0] < 0 or -1 < al.coord[i, 1] < 0]
    below = [i for i in idx["exact"] if (al.coord[i] != np.round(al.coord[i])).any()]
    return dict(erased=float((~keep).mean()), flips_radius=int((keep != keep_r1).sum()), flips_border=int((keep != keep_c).sum()),
                flips_floor_negative=int((keep[neg] != keep_fl[neg]).sum()), flips_floor_exact=int((keep[below] != keep_fl[below]).sum()))


def refine_ok(c):
    return (0.1 <= c["erased"] <= 0.9 and c["flips_radius"] >= 1 and c["flips_border"] >= 1 and c["flips_floor_negative"] >= 1 and
            c["flips_floor_exact"] >= 1)


def refine_case(H, W, r):
    """(alignment with the case's frame, group indices).  r = 0 is degenerate by construction: a one-tap window has range 0, so every
    point is erased for any positive event_diff; the discrimination conditions are asserted for r >= 1"""
    al, idx = refine_points(H, W)
    return sc.with_frame(al, refine_frame(H, W, r, REFINE_SEEDS.get((H, W, r), 0))), idx


# -- clean -------------------------------------------------------------------------------------------------------------------------
CLEAN_THRESHOLDS = (0.2, 0.7)


def clean_weights(seed, n):
    """uniform weights in [0, 1), none within 1e-6 of a threshold after rounding to fp32"""
    w = np.random.default_rng([seed, 0xC1]).uniform(0.0, 1.0, size=n)
    w32 = w.astype(np.float32).astype(np.float64)
    for t in CLEAN_THRESHOLDS:
        w = np.where(np.abs(w32 - t) <= 2e-6, t + 1e-3, w)
    return w


# -- projection --------------------------------------------------------------------------------------------------------------------
PROJ_N = 400


def _quat(axis, angle):
    return importlib.import_module("slam-eds_amd.synth").quat_from_axis_angle(axis, angle)


def projection_alignment(cam, H, W):
    """PROJ_N sub-pixel points plus EDGE_PIXELS under `cam`, inverse depths in [0.25, 5.15]"""
    key = ("kfp-proj", cam, H, W)
    if key not in ic._cache:
        al = ic.camera_alignment(6100 + 3 * H + W, H, W, PROJ_N, cam, pixels="subpixel", extra=ic.EDGE_PIXELS(H, W))
        idp = np.random.default_rng([H, W, 0xD9]).uniform(0.25, 5.15, size=al.N)
        ic._cache[key] = ic.replace(al, idp=idp)
    return ic._cache[key]


def projection_cases():
    """(name, cam, H, W, T7, K_dst, (dst_H, dst_W)): the camera comes towards the points (the cloud spreads through all four sides and
    the nearest points end behind it), with a roll and a shift; a destination camera and size other than the slot's"""
    out = []
    for cam, (H, W), roll in (("tall", (83, 61), 0.15), ("wide", (61, 83), -0.2)):
        T7 = np.concatenate([[0.05, -0.04, -0.2], _quat([0.1, -0.2, 1.0], roll)])
        fx, fy, cx, cy = ic.camera(cam, H, W)
        out.append((f"{cam}-own", cam, H, W, T7, None, None))
        out.append((f"{cam}-other", cam, H, W, T7, (1.1 * fx, 0.9 * fy, cx + 3.3, cy - 2.7), (H + 11, W + 5)))
    return out


def behind_case():
    """the camera jumps THROUGH the cloud: most points end behind it (Z' <= 0) and many of those still land in the frame, mirrored —
    the reference keeps them with their non-positive inverse depth, and so does the library"""
    return ("tall-behind", "tall", 83, 61, np.concatenate([[0.01, 0.02, -3.0], _quat([0.3, 0.1, 1.0], 0.05)]), None, None)


def edge_exact_case():
    """points that land EXACTLY on the destination frame's edges, so that `<` and `>=` are told from `<=` and `>`: K = (125, 125, 79.5,
    59.5) on 120 x 160, normalised coordinates 0 and +-2^-k, the identity transform (d a / d = a exactly), K_dst = (100, 80, 25, 20)
    and a 40 x 75 destination.  px = 100 a + 25 is 75 (out), 0 (in), 50, 25; py = 80 b + 20 is 40 (out), 0 (in), 30, 20.
    Returns (alignment, T7, K_dst, (dst_H, dst_W), expected keep mask)"""
    synth = importlib.import_module("slam-eds_amd.synth")
    H, W, K = 120, 160, (125.0, 125.0, 79.5, 59.5)
    ab = np.array([(0.5, 0.0), (-0.25, 0.0), (0.25, 0.25), (0.0, -0.25), (0.25, 0.125), (0.0, 0.0), (0.5, 0.25), (-0.25, -0.25),
                   (-0.5, 0.0), (0.0, -0.5)])
    keep = np.array([False, True, False, True, True, True, False, True, False, False])
    n = len(ab)
    rng = np.random.default_rng(0xE6)
    al = synth.Alignment(H=H, W=W, fx=K[0], fy=K[1], cx=K[2], cy=K[3], norm_coord=np.ascontiguousarray(ab), grad=rng.standard_normal((n, 2)),
                         idp=rng.uniform(0.3, 1.0, size=n), weights=np.ones(n), frame=rng.standard_normal((H, W)),
                         coord=np.column_stack([K[0] * ab[:, 0] + K[2], K[1] * ab[:, 1] + K[3]]))
    return al, np.array([0, 0, 0, 0, 0, 0, 1.0]), (100.0, 80.0, 25.0, 20.0), (40, 75), keep


def projection_inputs(case, mu=None, T7=None):
    """what the oracle takes for a case on an unseeded slot (mu: the seeds' of a seeded one; T7: the slot's solved pose)"""
    name, cam, H, W, T, K_dst, size = case
    al = projection_alignment(cam, H, W)
    K = (al.fx, al.fy, al.cx, al.cy)
    return dict(kpix=kp.slot_pixels(al.norm_coord, *K), mu=sc.f32(al.idp) if mu is None else np.asarray(mu, np.float64), K=K,
                T7=T if T7 is None else T7, K_dst=K if K_dst is None else K_dst, dst_size=(H, W) if size is None else size)


def projection_distance(inp):
    """the oracle's distance from the same formulas in np.longdouble over the points BOTH keep: (max |dxy| px, max |didp| / |idp|)"""
    a, b = kp.project(**inp), kp.project(**inp, dtype=np.longdouble)
    both = a["keep"] & b["keep"]
    if not both.any():
        return 0.0, 0.0
    dxy = max(float(np.abs(a["px"][both] - b["px"][both]).max()), float(np.abs(a["py"][both] - b["py"][both]).max()))
    return dxy, float((np.abs(a["idp"][both] - b["idp"][both]) / np.abs(b["idp"][both])).max())


def projection_allowance(extra=()):
    """4 x the largest distance over projection_cases() and `extra` inputs (as tests/test_depth_oracle.py sets its allowances)"""
    d = [projection_distance(projection_inputs(c)) for c in projection_cases() + [behind_case()]] + [projection_distance(e) for e in extra]
    return 4.0 * max(x for x, _ in d), 4.0 * max(y for _, y in d)
