"""Cases for include/eds_hip_map.h: windows of points under real-valued poses, the destination keyframes their depth maps are made
for, immature points and slot points.  Shapes are the smallest at which the kernels can go wrong: totals 0, 1, 63, 64, 65, one below, at
and above the compacting workgroup's sweep (``chunk`` points), two sweeps plus one, hosts without points at the start, in the middle
and at the end, and one window of 20 000 points.  Every case that is not deliberately degenerate is checked here, on the numpy oracle
alone, to keep at least one point and drop at least one in every map."""
import numpy as np

import np_map_oracle as mo

f32 = np.float32
WIN_H, WIN_W = 48, 64
CALIB = np.array([55.3, 54.1, 31.7, 23.2], f32)


def rot(axis, angle):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(R, t):
    """12 doubles, rows of [R | t]"""
    return np.concatenate([np.asarray(R, float), np.asarray(t, float).reshape(3, 1)], axis=1).reshape(12)


def inverse(T):
    R, t = T.reshape(3, 4)[:, :3], T.reshape(3, 4)[:, 3]
    return pose(R.T, -R.T @ t)


def random_pose(rng, angle=0.08, shift=0.2):
    return pose(rot(rng.normal(size=3), rng.uniform(-angle, angle)), rng.uniform(-shift, shift, 3))


# destination keyframes: (dst_H, dst_W) differ from the window's 48 x 64, one has H > W; K_dst crops the window's field of view
DST_SIZES = ((56, 40), (30, 70), (48, 64))


def destinations(rng, count, dst_H, dst_W):
    T = np.stack([inverse(random_pose(rng, 0.1, 0.25)) for _ in range(count)])
    K = np.stack([[rng.uniform(1.0, 1.3) * dst_W, rng.uniform(1.3, 1.7) * dst_H, rng.uniform(0.3, 0.6) * dst_W, rng.uniform(0.35, 0.65) * dst_H]
                  for _ in range(count)])
    return T, K


def window_case(name, per_host, seed, mask=None, count=1, size=0, degenerate=False):
    rng = np.random.default_rng(seed)
    F, n = len(per_host), int(sum(per_host))
    host = np.repeat(np.arange(F), per_host).astype(np.int32)
    uv = np.stack([rng.uniform(2, WIN_W - 3, n), rng.uniform(2, WIN_H - 3, n)], axis=1).astype(f32)
    uv[::3] = np.round(uv[::3])                                   # DSO's points sit on pixels; the tables hold floats
    ids = rng.uniform(0.3, 2.0, n).astype(f32)
    T_w_c = np.stack([random_pose(rng) for _ in range(F)])
    dst_H, dst_W = DST_SIZES[size]
    T_dst_w, K_dst = destinations(rng, count, dst_H, dst_W)
    c = dict(name=name, host=host, uv=uv, ids=ids, calib=CALIB.copy(), T_w_c=T_w_c, mask=(1 << F) - 1 if mask is None else mask,
             T_dst_w=T_dst_w, K_dst=K_dst, dst_H=dst_H, dst_W=dst_W, degenerate=degenerate)
    return check_mix(c)


def selected(c):
    return int(sum(np.sum(c["host"] == h) for h in range(len(c["T_w_c"])) if (c["mask"] >> h) & 1))


def check_mix(c):
    """on the oracle alone: every map of a case that is not degenerate keeps a point and drops a point"""
    if c["degenerate"]:
        return c
    nsel = selected(c)
    for b, m in enumerate(mo.window_depth_maps(c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"], c["mask"], c["T_dst_w"], c["K_dst"],
                                               c["dst_H"], c["dst_W"])):
        assert 0 < len(m["idp"]) < nsel, (c["name"], b, len(m["idp"]), nsel)
    return c


def window_cases(chunk):
    """`chunk`: the compacting kernels' sweep (edsmap::CHUNK)"""
    C = int(chunk)
    return [
        window_case("n0", [0, 0], 1, degenerate=True),
        window_case("n1", [0, 1], 2, degenerate=True),
        window_case("n63", [63, 0], 3),
        window_case("n64_gaps", [0, 20, 0, 30, 14, 0, 0, 0], 4, size=1),
        window_case("n65", [10, 10, 10, 10, 10, 5, 5, 5], 5, count=2),
        window_case("one_host", [10, 10, 10, 40, 10, 5, 5, 5], 6, mask=1 << 3),
        window_case("alternating", [10, 10, 10, 10, 10, 5, 5, 5], 7, mask=0b01010101, size=2),
        window_case("none", [10, 10, 10, 10, 10, 5, 5, 5], 8, mask=0, degenerate=True),
        window_case("all_and_more_bits", [10, 10, 10, 10, 10, 5, 5, 5], 9, mask=0xFFFFFFFF, count=5, size=1),
        window_case("chunk_minus_1", [C - 1, 3], 10),
        window_case("chunk", [C, 1], 11, size=2),
        window_case("chunk_plus_1", [C + 1, 0], 12, count=2, size=1),
        window_case("two_chunks_plus_1", [0, 2 * C + 1, 0, 7, 0, 0, C // 2, 0], 13),
        window_case("n20000", [3000, 0, 2500, 4100, 2900, 0, 3500, 4000], 14, count=2),
    ]


def degenerate_case():
    """inverse depths of 0, negative, denormal and NaN among ordinary ones; a destination at Z' == 0 of a point; Z' <= 0 in frame"""
    c = window_case("degenerate_idepths", [40, 0, 30], 21, count=2, degenerate=True)
    c["ids"][[0, 5, 41, 60]] = 0.0
    c["ids"][[1, 6, 42, 61]] = -c["ids"][[1, 6, 42, 61]]
    c["ids"][[2, 43]] = f32(1e-40)
    c["ids"][[3, 44]] = np.nan
    c["ids"][4] = -0.0
    return c


def plane_case():
    """identity poses and unit calibration, where the arithmetic is exact: a destination whose plane passes through points (Z' == 0),
    and points behind it (Z' < 0) that still land in the frame and are kept"""
    n = 12
    uv = np.stack([np.linspace(-6, 5, n), np.linspace(-4, 7, n)], axis=1).astype(f32)
    ids = np.array([1.0, 1.0, 2.0, 2.0, 0.5, 0.5, 1.0, 4.0, 4.0, 0.25, 1.0, 2.0], f32)
    eye = pose(np.eye(3), [0, 0, 0])
    T_dst = np.stack([pose(np.eye(3), [0, 0, -1.0]), pose(np.eye(3), [0, 0, -0.75])])      # Z' = 1 / ids - 1 and 1 / ids - 0.75
    K = np.array([[1.0, 1.0, 8.0, 8.0], [2.0, 2.0, 30.0, 30.0]])
    c = dict(name="plane", host=np.zeros(n, np.int32), uv=uv, ids=ids, calib=np.array([1, 1, 0, 0], f32), T_w_c=np.stack([eye, eye]), mask=3,
             T_dst_w=T_dst, K_dst=K, dst_H=60, dst_W=60, degenerate=True)
    m = mo.window_depth_maps(c["host"], uv, ids, c["calib"], c["T_w_c"], 3, T_dst, K, 60, 60)
    assert not np.isin(np.flatnonzero(ids == 1.0), m[0]["src"]).any()           # Z' == 0: x / 0 is +-inf or NaN, dropped
    assert (m[0]["idp"] < 0).any() and (m[1]["idp"] < 0).any()                   # Z' < 0 in frame: kept with its negative idp'
    return c


def edge_case():
    """The inlier rule's edges, constructed where the arithmetic is exact (identity rotations, unit focal lengths, idepth 1): a projection
    of exactly 0, the largest double below dst_W, exactly dst_W, just below 0, exactly dst_H, and exactly -0.0 (kept: -0.0 >= 0).
    Returns (case, expectations): per map, {table index: kept?}."""
    W, H = 40, 56
    below_W = np.nextafter(np.float64(W), 0.0)
    nz = -0.0
    # px = 1 * (u / 1) + cx_dst, py likewise: solve u, v for the wanted projection
    uv = np.array([[-8.0, 0.0],                                  # 0: map 0 px == 0            kept
                   [32.0, 0.0],                                  # 1: map 0 px == W            dropped
                   [np.nextafter(f32(-8.0), f32(-9.0)), 0.0],    # 2: map 0 px just below 0    dropped
                   [0.0, -8.0],                                  # 3: map 0 py == 0            kept
                   [0.0, 48.0],                                  # 4: map 0 py == H            dropped
                   [0.0, 1.0],                                   # 5: map 1 px == largest double below W: kept
                   [2.0 ** -47, 1.0],                            # 6: map 1 px == W exactly    dropped
                   [1.0, nz]], f32)                              # 7: map 2 py == -0.0         kept
    n = len(uv)
    eye = pose(np.eye(3), [0, 0, 0])
    # map 2: every term of the second row is -0.0, so that Y' = -0.0 survives the sums of both transforms
    neg = np.array([1, 0, 0, 0, nz, 1, nz, nz, 0, 0, 1, 0], float)
    T_dst = np.stack([eye, eye, neg])
    K = np.array([[1, 1, 8, 8], [1, 1, below_W, 8], [1, 1, 8, nz]], float)
    c = dict(name="edges", host=np.zeros(n, np.int32), uv=uv, ids=np.ones(n, f32), calib=np.array([1, 1, 0, 0], f32), T_w_c=np.stack([neg, eye]),
             mask=1, T_dst_w=T_dst, K_dst=K, dst_H=H, dst_W=W, degenerate=True)
    m = mo.window_depth_maps(c["host"], uv, c["ids"], c["calib"], c["T_w_c"], 1, T_dst, K, H, W)
    expect = [{0: True, 1: False, 2: False, 3: True, 4: False}, {5: True, 6: False}, {7: True}]
    at = lambda b, i: m[b]["xy"][list(m[b]["src"]).index(i)]      # noqa: E731
    for b, e in enumerate(expect):
        for i, kept in e.items():
            assert (i in m[b]["src"]) == kept, (b, i)
    assert at(0, 0)[0] == 0.0 and at(0, 3)[1] == 0.0 and at(1, 5)[0] == below_W and below_W < W
    py = at(2, 7)[1]
    assert py == 0.0 and np.signbit(py)                           # exactly -0.0, and kept
    return c, expect


def immature_case(name, per_host, seed, H=WIN_H, W=WIN_W, mask=None):
    """uv are pixels (eds_imm_create_points takes integers), some so close to the border that the pattern leaves the image: those points
    are dead.  Trace results: every lastTraceStatus, idepth_max NaN (DSO's initial state), a negative midpoint, a midpoint of 0."""
    rng = np.random.default_rng(seed)
    n = int(sum(per_host))
    uv = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.int32)
    lo = rng.uniform(0.05, 1.0, n).astype(f32)
    hi = (lo + rng.uniform(0.0, 1.0, n).astype(f32)).astype(f32)
    status = (np.arange(n) % 6).astype(np.int32)
    hi[1::7] = np.nan
    lo[2::11], hi[2::11] = -hi[2::11], -lo[2::11]
    lo[3::13], hi[3::13] = 0.0, 0.0
    lo[5::17] = -hi[5::17]                                        # midpoint +0: d_i = +inf, skipped
    return dict(name=name, per_host=list(per_host), uv=uv, idepth_min=lo, idepth_max=hi, status=status,
                T_w_c=np.stack([random_pose(rng) for _ in per_host]), calib=CALIB.copy(), mask=(1 << len(per_host)) - 1 if mask is None else mask)


def immature_cases(chunk):
    C = int(chunk)
    return [immature_case("imm_small", [0, 37, 0, 64, 1], 31), immature_case("imm_one_host", [50, 60, 70], 32, mask=0b010),
            immature_case("imm_chunks", [C + 1, 0, 2 * C + 1, C - 1], 33), immature_case("imm_none", [5, 5], 34, mask=0)]


def pattern_alive(uv, H, W):
    """which points an eds_imm reports alive: every pixel of the pattern (offsets -2 .. 2) has its bilinear cell inside the image"""
    return ((uv[:, 0] >= 2) & (uv[:, 0] <= W - 4) & (uv[:, 1] >= 2) & (uv[:, 1] <= H - 4)).astype(np.int32)


def slot_case(seed, n):
    rng = np.random.default_rng(seed)
    return dict(xn=rng.uniform(-0.6, 0.6, n).astype(f32), yn=rng.uniform(-0.4, 0.4, n).astype(f32), idp=rng.uniform(0.3, 2.0, n), T_w_kf=random_pose(rng))
