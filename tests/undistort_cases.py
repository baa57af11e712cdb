"""The committed cases of the undistorter: camera geometries at the smallest sizes at which each branch of the set-up can be taken, and
raw frames, G tables and vignettes built from fixed seeds with numpy alone.  What each geometry is there for is in ``covers``;
tests/test_undistort_oracle.py asserts, from the oracle alone, that it still does."""
from types import SimpleNamespace

import numpy as np

import np_undistort_oracle as uo


def _g(name, covers, *a, **k):
    return SimpleNamespace(name=name, covers=covers, g=uo.geometry(*a, **k))


def geometries():
    c = [
        # the five models, crop; 40 x 32 raw to 36 x 28: no multiple of the 64 x 4 workgroup tile
        _g("fov_crop_relative", ("relative", "crop"), uo.FOV, [0.535719308086809, 0.669566858850269, 0.493248545285398, 0.500408664348414, 0.897966326944875],
           40, 32, uo.CROP, 36, 28),
        _g("radtan_crop_absolute", ("absolute", "crop"), uo.RADTAN, [30.0, 31.0, 19.2, 15.7, -0.28, 0.07, 0.002, -0.0015], 40, 32, uo.CROP, 36, 28),
        _g("equidistant_crop", ("absolute", "crop"), uo.EQUIDISTANT, [24.0, 24.5, 19.4, 15.3, -0.013, 0.05, -0.08, 0.04], 40, 32, uo.CROP, 36, 28),
        _g("kb_crop", ("absolute", "crop"), uo.KB, [23.0, 23.5, 19.6, 15.8, 0.02, -0.01, 0.004, -0.001], 40, 32, uo.CROP, 36, 28),
        _g("pinhole_crop_relative", ("relative", "crop"), uo.PINHOLE, [0.75, 0.95, 0.49, 0.51, 0.0], 40, 32, uo.CROP, 36, 28),
        # the other two output modes, 37 x 29 to 37 x 29
        _g("radtan_given", ("absolute", "given"), uo.RADTAN, [30.0, 31.0, 18.2, 14.1, -0.2, 0.05, 0.001, 0.0005], 37, 29, uo.GIVEN, 37, 29,
           out_pars=(0.9, 1.15, 0.5, 0.5, 0.0)),
        _g("fov_none", ("absolute", "none"), uo.FOV, [30.0, 31.0, 18.2, 14.1, 0.6], 37, 29, uo.NONE, 37, 29),
        # crops that shrink one dimension only: the other one's centre line ends with the +-5 the samples cover, inside the image
        _g("radtan_crop_left_right", ("crop", "left_right_only"), uo.RADTAN, [30.0, 2.5, 19.5, 15.5, -0.002, 0.0, 0.0001, 0.0], 40, 32, uo.CROP, 36, 28),
        _g("radtan_crop_top_bottom", ("crop", "top_bottom_only"), uo.RADTAN, [3.2, 30.0, 19.5, 15.5, -0.002, 0.0, 0.0, 0.0001], 40, 32, uo.CROP, 36, 28),
        # a principal point far outside the image: both centre lines stay outside, the range is 0, the loop runs out
        _g("pinhole_crop_fails", ("crop_fails",), uo.PINHOLE, [30.0, 30.0, 5000.0, 15.5, 0.0], 40, 32, uo.CROP, 36, 28),
        # portrait: the map's test iy < wOrg - 1 throws rows away that the raw image has
        _g("fov_crop_portrait", ("crop", "portrait_rows_lost"), uo.FOV, [30.0, 31.0, 15.7, 19.2, 0.7], 32, 40, uo.CROP, 28, 36),
        # landscape, an output that looks further down than the raw image reaches: h_org - 1 <= iy < w_org - 1, defined rule (1)
        _g("pinhole_given_rule", ("given", "rule_pixels"), uo.PINHOLE, [30.0, 30.0, 19.5, 15.5, 0.0], 40, 32, uo.GIVEN, 36, 28,
           out_pars=(0.75, 0.5, 0.5, 0.5, 0.0)),
    ]
    return {x.name: x for x in c}


def grid_geometry():
    """one 640 x 480 case: more than one workgroup in every grid dimension"""
    return _g("fov_crop_640x480", ("crop",), uo.FOV, [0.535719308086809, 0.669566858850269, 0.493248545285398, 0.500408664348414, 0.897966326944875],
              640, 480, uo.CROP, 640, 480)


def handover_geometry():
    """72 x 56 to 64 x 48: the smallest plane the selector (32 x 32 blocks) and a three-level coarse tracker both take"""
    return _g("radtan_crop_72x56", ("crop",), uo.RADTAN, [55.0, 56.0, 35.2, 27.6, -0.25, 0.06, 0.001, -0.0008], 72, 56, uo.CROP, 64, 48)


def raw_frames(count, h, w, seed, dtype=np.uint8):
    """smooth random frames over the whole range of `dtype`, both ends of the range included in every frame"""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((count, h, w), dtype)
    for k in range(count):
        img = np.full((h, w), 0.5)
        for _ in range(6):
            fx, fy = rng.uniform(-0.7, 0.7, 2)
            img += 0.12 * np.sin(fx * x + fy * y + rng.uniform(0, 6.28))
        img += rng.normal(0, 0.05, (h, w))
        f = np.clip(img, 0, 1) * top
        f[rng.integers(h), rng.integers(w)] = 0
        f[rng.integers(h), rng.integers(w)] = top
        f[h - 1, w - 1] = top * 0.75          # the last row's last pixel: a tap of xxi = w - 2, yyi = h - 2
        out[k] = f.astype(dtype)
    return out


def gamma_table(depth=256, seed=5):
    """an inverse response that is strictly increasing with a varying slope, NOT on the 0 .. 255 scale (the constructor rescales it)"""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.2, 1.8, depth) * (1.0 + 0.8 * np.sin(np.arange(depth) * (6.0 / depth)))
    return (3.0 + np.cumsum(np.abs(steps) + 0.05)).astype(np.float32)


def vignette(h, w, dtype=np.uint16, zero_at=None):
    """a radial fall-off; zero_at = (y, x): one entry that is 0, whose inverse is inf"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((x - 0.48 * w) / w) ** 2 + ((y - 0.53 * h) / h) ** 2
    v = np.iinfo(dtype).max * (0.97 - 1.3 * r2)
    v = np.clip(v, 1, np.iinfo(dtype).max).astype(dtype)
    if zero_at is not None:
        v[zero_at] = 0
    return v


def same_bits(a, b):
    """two float32 arrays bit for bit; a NaN equals a NaN whatever its sign or payload (x86 and gfx950 differ in the default NaN's sign)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def _s(name, geometry, **k):
    d = dict(dtype=np.uint8, exposures=(0.02,), factor=1.0, mode=2, use_exposure=1, g_depth=256, vignette_dtype=np.uint16, zero_at=None, seed=1)
    d.update(k)
    return SimpleNamespace(name=name, geometry=geometry, **d)


def scenarios():
    """per-frame cases over the geometries above: (geometry, raw type, exposures — one frame each —, factor, settings, calibration).
    g_depth None: no photometric calibration is set (the reference's !valid)."""
    c = [
        # one call takes both branches (exposure <= 0 in the middle); a zero vignette entry under a raw 0 gives 0 * inf = NaN
        _s("mode2_u8_batch_nan", "fov_crop_relative", exposures=(0.02, 0.0, 0.013), factor=0.8, zero_at=(16, 20), seed=2),
        _s("mode1_u8_vignette8", "radtan_crop_absolute", mode=1, vignette_dtype=np.uint8, g_depth=300, seed=3),
        _s("mode0_u8_factor", "equidistant_crop", mode=0, factor=1.25, seed=4),
        _s("no_calibration", "kb_crop", g_depth=None, exposures=(0.01, 0.03), factor=0.5, seed=5),
        _s("use_exposure_off_last_tap", "pinhole_crop_relative", use_exposure=0, exposures=(0.5,), seed=6),
        _s("passthrough", "fov_none", exposures=(0.02, -1.0), factor=2.0, seed=7),
        _s("given", "radtan_given", seed=8),
        _s("u16_g65536_rule", "pinhole_given_rule", dtype=np.uint16, g_depth=65536, exposures=(0.01, -1.0), factor=1.0 / 256, seed=9),
        _s("u16_plain_portrait", "fov_crop_portrait", dtype=np.uint16, g_depth=None, factor=1.0 / 256, seed=10),
        _s("left_right", "radtan_crop_left_right", mode=1, seed=11),
        _s("top_bottom", "radtan_crop_top_bottom", seed=12),
    ]
    return {x.name: x for x in c}


def scenario_inputs(sc, geometry=None):
    """(geometry dict, raw frames, G or None, vignette or None) of a scenario"""
    g = (geometry or geometries()[sc.geometry]).g
    raw = raw_frames(len(sc.exposures), g["h_org"], g["w_org"], sc.seed, sc.dtype)
    if sc.zero_at is not None:
        raw[:, sc.zero_at[0], sc.zero_at[1]] = 0
    if sc.g_depth is None:
        return g, raw, None, None
    return g, raw, gamma_table(sc.g_depth, sc.seed), vignette(g["h_org"], g["w_org"], sc.vignette_dtype, sc.zero_at)


_expected = {}


def expected(sc, geometry=None):
    """the oracle's answer for a scenario, computed once: dict(setup, planes count x h x w, exposures, branches)"""
    key = (sc.name, None if geometry is None else geometry.name)
    if key not in _expected:
        g, raw, G, vig = scenario_inputs(sc, geometry)
        su = uo.setup(g)
        st = dict(photometric_calibration=sc.mode, use_exposure=sc.use_exposure)
        ph = None if G is None else uo.photometric(G, vig, sc.mode)
        res = [uo.undistort(su, ph, raw[k], e, sc.factor, st) for k, e in enumerate(sc.exposures)]
        _expected[key] = dict(setup=su, planes=np.stack([r[0] for r in res]), exposures=np.array([r[1] for r in res], np.float32),
                              branches=[r[2] for r in res], raw=raw, G=G, vignette=vig, photometric=ph)
    return _expected[key]


def run_scenario(sc, make, geometry=None, **process_kw):
    """the scenario on an object with the interface of undistort.Undistorter (`make(geometry dict, slots)` creates it):
    (planes, exposures out, the object)"""
    g, raw, G, vig = scenario_inputs(sc, geometry)
    u = make(g, len(sc.exposures))
    if G is not None:
        u.set_photometric(G, vig)
    u.set_settings(photometric_calibration=sc.mode, use_exposure=sc.use_exposure)
    e = u.process(raw, sc.exposures, factor=sc.factor, **process_kw)
    return np.stack([u.get_image(k) for k in range(len(sc.exposures))]), e, u
