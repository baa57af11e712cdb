"""Seeded scenes for the immature-point tests (tests/test_immature_oracle.py, tests/test_immature_gpu.py), all small.

A scene is a textured plane Z = Z0 seen by pinhole cameras with fx != fy and an off-centre principal point: host frames at slightly
different poses (each rotated a little about all three axes, so that hostToFrame_KRKi is not the identity and fx / fy shows in it) and
four target frames along a translating path, so that the intervals narrow from UNINITIALIZED.  Frames are smooth texture plus noise on
DSO's 0 .. 255 scale.  What the cases add on purpose:
  - target 1 has a NaN patch (energies take the 1e5 branch; a point can go OUTLIER there);
  - targets 1 and 2 carry a block of foreign texture at the same place (OUTLIER twice in a row: OOB);
  - target 0 has a FLAT patch over a low-contrast part of host 0: every step of a line there has the same taps, so energies tie exactly
    and the arg-min's strict < decides which step wins;
  - points on the border (their pattern leaves the image: dead), N in {1, 63, 64, 65, 300}, hosts in {1, 3, 7};
  - long lines: 160 x 120 with max_pix_search raised so that numSteps is 64, 65 and the cap of 99."""
import numpy as np

F = np.float32


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def precalc32(K4, R, t, aff=(1.0, 0.0)):
    """hostToFrame_KRKi, hostToFrame_Kt, hostToFrame_affine as DSO's traceNewCoarse forms them: float matrices, float products"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=F)
    Ki = np.linalg.inv(K.astype(np.float64)).astype(F)
    KRKi = (K @ np.asarray(R, dtype=F)) @ Ki
    Kt = K @ np.asarray(t, dtype=F)
    return KRKi.astype(F), Kt.astype(F), np.asarray(aff, dtype=F)


class Scene:
    def __init__(self, seed, H, W, K4, Z0=2.0):
        self.rng = np.random.default_rng(seed)
        self.H, self.W, self.K4, self.Z0 = H, W, K4, Z0
        r = self.rng
        self.waves = [(r.uniform(8, 20) * r.choice([-1, 1]), r.uniform(8, 20) * r.choice([-1, 1]), r.uniform(0, 6.28), a) for a in (38, 26, 18, 10)]

    def texture(self, X, Y):
        out = np.full(X.shape, 120.0)
        for a, b, ph, amp in self.waves:
            out += amp * np.sin(a * X + b * Y + ph)
        return out

    def render(self, R_wc, p, noise=1.0):
        fx, fy, cx, cy = self.K4
        v, u = np.mgrid[0:self.H, 0:self.W].astype(np.float64)
        d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ R_wc.T
        s = (self.Z0 - p[2]) / d[..., 2]
        X, Y = p[0] + s * d[..., 0], p[1] + s * d[..., 1]
        img = self.texture(X, Y) + noise * self.rng.standard_normal(X.shape)
        return np.clip(img, 0, 255).astype(F)


class Case:
    """hosts: dicts image, uv, type, idepth | None, distance | None; targets: images; steps: per target k one list with, for every host,
    (KRKi, Kt, aff, KRKi with fx taken for fy)"""
    def __init__(self, name, H, W, K4, prm):
        self.name, self.H, self.W, self.K4, self.prm = name, H, W, K4, prm
        self.hosts, self.targets, self.steps = [], [], []


def _points(rng, H, W, n, border):
    uv = np.stack([rng.integers(6, W - 6, n), rng.integers(6, H - 6, n)], axis=1)
    k = min(border, n // 8)
    if k:                                             # some on the border: the pattern leaves the image
        uv[:k, 0] = rng.choice([0, 1, W - 2, W - 1], k)
        uv[k:2 * k, 1] = rng.choice([0, 1, H - 2, H - 1], k)
    return uv.astype(np.int32)


def make_case(name, seed, H, W, K4, counts, path, seeded, prm, special=False, box=None):
    sc = Scene(seed, H, W, K4)
    rng = sc.rng
    c = Case(name, H, W, K4, prm)
    poses = []
    for h, n in enumerate(counts):
        R = rot(*(rng.uniform(-0.02, 0.02, 2)), rng.uniform(-0.06, 0.06))
        p = np.append(rng.uniform(-0.01, 0.01, 2), rng.uniform(-0.02, 0.02))
        poses.append((R, p))
        img = sc.render(R, p)
        if special and h == 0:                        # low contrast around 200 where target 0 will be flat
            yy, xx = np.mgrid[0:H, 0:W]
            img[30:56, 44:84] = (200 + 4 * np.sin(0.9 * xx + 0.7 * yy))[30:56, 44:84].astype(F)
        uv = _points(rng, H, W, n, 4)
        if box is not None and n > 8:                 # long lines need room: keep most points where the line fits
            uv[8:, 0] = rng.integers(box[0], box[1], n - 8)
            uv[8:, 1] = rng.integers(box[2], box[3], n - 8)
        if special and h == 0:
            uv[40:70, 0] = rng.integers(52, 76, 30)
            uv[40:70, 1] = rng.integers(36, 50, 30)
        host = dict(image=img, uv=uv, type=rng.choice([1.0, 2.0, 4.0], n).astype(F), idepth=None, distance=None)
        if seeded:
            host["idepth"] = (1.0 / sc.Z0 * (1 + 0.06 * rng.standard_normal(n))).astype(F)
            host["distance"] = rng.uniform(0.05, 1.6, n)
        c.hosts.append(host)
    for k in range(4):
        Rt = rot(*(rng.uniform(-0.01, 0.01, 2)), rng.uniform(-0.03, 0.03))
        pt = np.asarray(path, dtype=np.float64) * (k + 1)
        img = sc.render(Rt, pt)
        if special:
            if k == 0:
                img[24:62, 36:92] = 200.0
            if k == 1:
                img[8:26, 10:34] = np.nan
            if k in (1, 2):
                yy, xx = np.mgrid[0:H, 0:W]
                img[44:68, 6:40] = (128 + 100 * np.sin(2.1 * xx) * np.cos(1.7 * yy))[44:68, 6:40].astype(F)
        c.targets.append(img)
        step = []
        for (Rh, ph) in poses:
            R = Rt.T @ Rh
            t = Rt.T @ (ph - pt)
            aff = (1.0 + 0.01 * k, -0.5 * k)
            KRKi, Kt, a = precalc32(K4, R, t, aff)
            wrong, _, _ = precalc32((K4[0], K4[0], K4[2], K4[3]), R, t, aff)
            step.append((KRKi, Kt, a, wrong))
        c.steps.append(step)
    return c


_CASES = None


def cases():
    """name -> Case, built once"""
    global _CASES
    if _CASES is None:
        KA, KB, KL = (82.0, 77.0, 50.5, 33.25), (61.0, 66.0, 33.75, 51.5), (130.0, 122.0, 83.5, 57.25)
        cs = [
            make_case("x3_gn3", 11, 72, 96, KA, [300, 65, 1], (0.022, 0.004, 0.003), False, dict(), special=True),
            make_case("y7_gn3_seeded", 12, 96, 72, KB, [63, 64, 65, 1, 63, 64, 65], (-0.003, 0.03, -0.002), True, dict()),
            make_case("d1_gn0_seeded", 13, 72, 96, KA, [300], (0.018, -0.017, 0.0), True, dict(trace_gn_iterations=0)),
            make_case("d1_gn0", 14, 96, 72, KB, [64], (-0.02, -0.02, 0.004), False, dict(trace_gn_iterations=0)),
            make_case("long64", 15, 120, 160, KL, [63], (-0.2, 0.01, 0.0), False, dict(max_pix_search=62.5 / 280), box=(8, 80, 20, 100)),
            make_case("long65", 16, 120, 160, KL, [63], (-0.2, -0.01, 0.0), False, dict(max_pix_search=63.5 / 280), box=(8, 80, 20, 100)),
            make_case("long99", 17, 120, 160, KL, [63], (-0.3, 0.0, 0.0), False, dict(max_pix_search=0.4), box=(8, 40, 20, 100)),
        ]
        _CASES = {c.name: c for c in cs}
    return _CASES


_ORACLE = {}


def oracle_run(name, **variant):
    """The oracle over a whole case, computed once per (case, variant) and never modified by the tests: images, the points after the
    constructor and after every trace, the summaries and the branch statistics.  variant: argmin_le, mul_step (np_immature_oracle.trace)
    and wrong_fy (the caller's KRKi formed with fx for fy)."""
    key = (name,) + tuple(sorted(variant.items()))
    if key not in _ORACLE:
        import np_immature_oracle as no
        c = cases()[name]
        prm = no.params(**c.prm)
        wrong = variant.pop("wrong_fy", False)
        himg = [no.make_image(h["image"]) for h in c.hosts]
        timg = [no.make_image(t) for t in c.targets]
        P = [no.construct(himg[i], h["uv"], h["type"], h["idepth"], h["distance"], prm) for i, h in enumerate(c.hosts)]
        after = [[no.copy_points(p) for p in P]]
        stats, sums = [], []
        for k, step in enumerate(c.steps):
            stats.append([no.trace(P[i], timg[k], s[3] if wrong else s[0], s[1], s[2], prm, **variant) for i, s in enumerate(step)])
            sums.append(np.stack([no.summary(p) for p in P]))
            after.append([no.copy_points(p) for p in P])
        _ORACLE[key] = dict(prm=prm, host_images=himg, target_images=timg, after=after, stats=stats, summaries=sums)
    return _ORACLE[key]


FIELDS = ("idepth_min", "idepth_max", "quality", "status", "last_uv", "last_interval")
