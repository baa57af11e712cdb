"""A literal numpy restatement of dso::Undistort with its PhotometricUndistorter, written from the reference's lines
(src/utils/Undistort.cpp; line numbers below) and independent of csrc/eds_undistort.hpp: readFromFile from :782 on, makeOptimalK_crop
(:580-700), the five distortCoordinates (:961-1225), the constructor of PhotometricUndistorter after its file reads (:79-170),
processFrame<T> (:206-244) and undistort<T> (:378-474).

Every array is float32 or float64 exactly where the reference's variable is float or double, every scalar is wrapped so that numpy
cannot promote it, and expressions keep the reference's order.  tanf, atanf, atan2f and sqrtf are the C LIBRARY's, called through
ctypes one value at a time: numpy's own float32 arctan differs from glibc's atanf in a quarter of all inputs, and the library under
test builds its map with the C library's.  With them every comparison against this oracle is bit for bit, the set-up included.

One rule is not the reference's (include/eds_hip_undistort.h, defined rule 1): a map pixel the reference's test lets through although
its taps would lie below the raw image (h_org - 1 <= iy < w_org - 1) is (-1, -1); ``setup`` counts them in ``rule_pixels``.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
D = np.float64
FOV, RADTAN, EQUIDISTANT, KB, PINHOLE = range(5)
CROP, NONE, GIVEN, FULL = range(4)
U8, U16 = 0, 1
# reference src/utils/settings.cpp:117-118
SETTINGS = dict(photometric_calibration=2, use_exposure=1)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("tanf", "atanf", "sqrtf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


class CropFailed(Exception):
    """the reference prints FAILED TO COMPUTE GOOD CAMERA MATRIX and calls exit(1)"""


def _each(fn, a, *more):
    a = np.asarray(a, F)
    return np.array([fn(v, *more) for v in a.ravel().tolist()], F).reshape(a.shape)


def tanf(a):
    return _each(_libm.tanf, a)


def atanf(a):
    return _each(_libm.atanf, a)


def sqrtf(a):
    return _each(_libm.sqrtf, a)


def atan2f_1(a):
    return _each(_libm.atan2f, a, 1.0)


def geometry(model, pars, w_org, h_org, out_mode, w, h, out_pars=(0, 0, 0, 0, 0)):
    p = np.zeros(8, D)
    p[:len(pars)] = pars
    return dict(model=int(model), pars=p, w_org=int(w_org), h_org=int(h_org), out_mode=int(out_mode), out_pars=np.asarray(out_pars, F),
                w=int(w), h=int(h))


def distort(model, parsOrg, K, in_x, in_y):
    """distortCoordinates of the five classes; parsOrg and K are doubles, everything else float"""
    x, y = np.asarray(in_x, F), np.asarray(in_y, F)
    fx, fy, cx, cy = (F(parsOrg[i]) for i in range(4))
    ofx, ofy, ocx, ocy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    with np.errstate(all="ignore"):
        ix = (x - ocx) / ofx
        iy = (y - ocy) / ofy
        if model == FOV:                                                                    # :961-997
            dist = F(parsOrg[4])
            d2t = F(2.0) * tanf(dist / F(2.0))[()]
            r = sqrtf(ix * ix + iy * iy)
            fac = np.where((r == 0) | (dist == 0), F(1), atanf(r * d2t) / (dist * r)).astype(F)
            return fx * fac * ix + cx, fy * fac * iy + cy
        if model == RADTAN:                                                                 # :1017-1060
            k1, k2, r1, r2 = (F(parsOrg[i]) for i in range(4, 8))
            mx2_u = ix * ix
            my2_u = iy * iy
            mxy_u = ix * iy
            rho2_u = mx2_u + my2_u
            rad_dist_u = k1 * rho2_u + k2 * rho2_u * rho2_u
            x_dist = (((ix + ix * rad_dist_u).astype(D) + (2.0 * D(r1)) * mxy_u.astype(D)) + D(r2) * (rho2_u.astype(D) + 2.0 * mx2_u.astype(D))).astype(F)
            y_dist = (((iy + iy * rad_dist_u).astype(D) + (2.0 * D(r2)) * mxy_u.astype(D)) + D(r1) * (rho2_u.astype(D) + 2.0 * my2_u.astype(D))).astype(F)
            return fx * x_dist + cx, fy * y_dist + cy
        if model == EQUIDISTANT:                                                            # :1077-1119
            k1, k2, k3, k4 = (F(parsOrg[i]) for i in range(4, 8))
            r = sqrtf(ix * ix + iy * iy)
            theta = atanf(r)
            theta2 = theta * theta
            theta4 = theta2 * theta2
            theta6 = theta4 * theta2
            theta8 = theta4 * theta4
            thetad = theta * (F(1) + k1 * theta2 + k2 * theta4 + k3 * theta6 + k4 * theta8)
            scaling = np.where(r.astype(D) > 1e-8, thetad / r, F(1)).astype(F)
            return fx * ix * scaling + cx, fy * iy * scaling + cy
        if model == KB:                                                                     # :1136-1183
            k0, k1, k2, k3 = (F(parsOrg[i]) for i in range(4, 8))
            Xsq_plus_Ysq = ix * ix + iy * iy
            sqrt_Xsq_Ysq = sqrtf(Xsq_plus_Ysq)
            theta = atan2f_1(sqrt_Xsq_Ysq)
            theta2 = theta * theta
            theta3 = theta2 * theta
            theta5 = theta3 * theta2
            theta7 = theta5 * theta2
            theta9 = theta7 * theta2
            r = theta + k0 * theta3 + k1 * theta5 + k2 * theta7 + k3 * theta9
            small = sqrt_Xsq_Ysq.astype(D) < 1e-6
            ox = np.where(small, fx * ix + cx, (r / sqrt_Xsq_Ysq) * fx * ix + cx).astype(F)
            oy = np.where(small, fy * iy + cy, (r / sqrt_Xsq_Ysq) * fy * iy + cy).astype(F)
            return ox, oy
        assert model == PINHOLE                                                             # :1201-1225
        return fx * ix + cx, fy * iy + cy


def _line_range(t, vals, limit):
    """:596-603: the first valid sample sets min unless min is still 0 after it — a valid sample AT 0 is passed over — the last sets max"""
    lo, hi = F(0), F(0)
    with np.errstate(invalid="ignore"):
        ok = (vals > 0) & (vals < F(limit))
    for v in t[ok].tolist():
        if lo == 0:
            lo = F(v)
        hi = F(v)
    return lo, hi


def make_optimal_K_crop(g, info):
    """:580-700.  Raises CropFailed where the reference exits."""
    w, h, wOrg, hOrg = g["w"], g["h"], g["w_org"], g["h_org"]
    K = np.eye(3)
    t = (np.arange(100000, dtype=F) - F(50000.0)) / F(10000.0)
    zero = np.zeros(100000, F)
    tgX, _ = distort(g["model"], g["pars"], K, t, zero)
    minX, maxX = _line_range(t, tgX, wOrg - 1)
    _, tgY = distort(g["model"], g["pars"], K, zero, t)
    minY, maxY = _line_range(t, tgY, hOrg - 1)
    minX, maxX, minY, maxY = (F(D(v) * 1.01) for v in (minX, maxX, minY, maxY))
    info["range"] = (minX, maxX, minY, maxY)
    shrinks = [0, 0, 0, 0]
    yv, xv = np.arange(h, dtype=F), np.arange(w, dtype=F)
    oobLeft = oobRight = oobTop = oobBottom = True
    iteration = 0
    while oobLeft or oobRight or oobTop or oobBottom:
        with np.errstate(all="ignore"):
            ry = minY + (maxY - minY) * yv / (F(h) - F(1.0))
            left, _ = distort(g["model"], g["pars"], K, np.full(h, minX, F), ry)
            right, _ = distort(g["model"], g["pars"], K, np.full(h, maxX, F), ry)
            oobLeft = bool(np.any(~((left > 0) & (left < F(wOrg - 1)))))
            oobRight = bool(np.any(~((right > 0) & (right < F(wOrg - 1)))))
            rx = minX + (maxX - minX) * xv / (F(w) - F(1.0))
            _, top = distort(g["model"], g["pars"], K, rx, np.full(w, minY, F))
            _, bottom = distort(g["model"], g["pars"], K, rx, np.full(w, maxY, F))
            oobTop = bool(np.any(~((top > 0) & (top < F(hOrg - 1)))))
            oobBottom = bool(np.any(~((bottom > 0) & (bottom < F(hOrg - 1)))))
        if (oobLeft or oobRight) and (oobTop or oobBottom):
            if (maxX - minX) > (maxY - minY):
                oobBottom = oobTop = False
            else:
                oobLeft = oobRight = False
        if oobLeft:
            minX = F(D(minX) * 0.995)
            shrinks[0] += 1
        if oobRight:
            maxX = F(D(maxX) * 0.995)
            shrinks[1] += 1
        if oobTop:
            minY = F(D(minY) * 0.995)
            shrinks[2] += 1
        if oobBottom:
            maxY = F(D(maxY) * 0.995)
            shrinks[3] += 1
        iteration += 1
        info["iterations"], info["shrinks"] = iteration, tuple(shrinks)
        if iteration > 500:
            raise CropFailed()
    with np.errstate(all="ignore"):
        K[0, 0] = (F(w) - F(1.0)) / (maxX - minX)
        K[1, 1] = (F(h) - F(1.0)) / (maxY - minY)
    K[0, 2] = D(-minX) * K[0, 0]
    K[1, 2] = D(-minY) * K[1, 1]
    return K


def setup(g):
    """readFromFile from :782 on: dict with K (3 x 3 doubles), mapx, mapy (h x w floats), passthrough, pars (after the rescale), and what
    the tests assert their cases on: relative, iterations, shrinks, range, rule_pixels, portrait_rows_lost"""
    assert g["out_mode"] != FULL, "makeOptimalK_full: assert(false)"
    g = dict(g, pars=np.array(g["pars"], D))
    p, w, h, wOrg, hOrg = g["pars"], g["w"], g["h"], g["w_org"], g["h_org"]
    info = dict(relative=False, iterations=0, shrinks=(0, 0, 0, 0), range=None, passthrough=False)
    if p[2] < 1 and p[3] < 1:                                                               # :782-798
        p[0] = p[0] * wOrg
        p[1] = p[1] * hOrg
        p[2] = p[2] * wOrg - 0.5
        p[3] = p[3] * hOrg - 0.5
        info["relative"] = True
    if g["out_mode"] == CROP:
        K = make_optimal_K_crop(g, info)
    elif g["out_mode"] == NONE:
        assert w == wOrg and h == hOrg
        K = np.eye(3)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = p[0], p[1], p[2], p[3]
        info["passthrough"] = True
    else:
        oc = np.asarray(g["out_pars"], F)
        K = np.eye(3)
        K[0, 0] = oc[0] * F(w)
        K[1, 1] = oc[1] * F(h)
        K[0, 2] = D(oc[2] * F(w)) - 0.5
        K[1, 2] = D(oc[3] * F(h)) - 0.5
    yy, xx = np.mgrid[0:h, 0:w]
    ix, iy = distort(g["model"], p, K, xx.astype(F).ravel(), yy.astype(F).ravel())         # :903-910
    ix, iy = ix.copy(), iy.copy()
    ix[ix == 0] = F(0.001)                                                                  # :920-923
    iy[iy == 0] = F(0.001)
    ix[ix == F(wOrg - 1)] = F(wOrg - 1.001)
    ix[iy == F(hOrg - 1)] = F(hOrg - 1.001)
    with np.errstate(invalid="ignore"):
        reference_test = (ix > 0) & (iy > 0) & (ix < F(wOrg - 1)) & (iy < F(wOrg - 1))     # :925
        rows_exist = iy < F(hOrg - 1)
        inside_image = (ix > 0) & (iy > 0) & (ix < F(wOrg - 1)) & rows_exist
    keep = reference_test & rows_exist
    info["rule_pixels"] = int(np.sum(reference_test & ~rows_exist))
    info["portrait_rows_lost"] = int(np.sum(inside_image & ~reference_test))
    mapx = np.where(keep, ix, F(-1)).astype(F).reshape(h, w)
    mapy = np.where(keep, iy, F(-1)).astype(F).reshape(h, w)
    return dict(info, K=K, mapx=mapx, mapy=mapy, pars=p, g=g)


def photometric(G, vignette, mode=2):
    """the constructor after its file reads (:79-170); None where it returns with valid == false over G"""
    G = np.asarray(G, F).copy()
    GDepth = G.size
    if GDepth < 256 or np.any(~(G[1:] > G[:-1])):
        return None
    mn, mx = G[0], G[-1]
    G = (255.0 * (G - mn).astype(D) / D(mx - mn)).astype(F)                                  # :101
    if mode == 0:
        G = (F(255.0) * np.arange(GDepth, dtype=F) / F(GDepth - 1)).astype(F)               # :106
    v = np.asarray(vignette)
    assert v.dtype in (np.uint8, np.uint16)
    with np.errstate(all="ignore"):
        maxV = F(max(0, int(v.max())))
        vignetteMap = v.astype(F) / maxV
        vignetteMapInv = F(1.0) / vignetteMap
    return dict(G=G, GDepth=GDepth, vignetteMapInv=vignetteMapInv.astype(F))


def process_frame(raw, ph, exposure, factor, settings=SETTINGS):
    """processFrame<T> (:206-244): the photometric plane and output->exposure_time; also which branch ran"""
    raw = np.asarray(raw)
    mode = settings["photometric_calibration"]
    exposure = F(exposure)
    with np.errstate(all="ignore"):
        if ph is None or exposure <= 0 or mode == 0:
            data = F(factor) * raw.astype(np.int32).astype(F)
            branch = "plain"
        else:
            data = ph["G"][raw.astype(np.int64)]
            if mode == 2:
                data = data * ph["vignetteMapInv"]
            branch = "photometric"
    return data.astype(F), (exposure if settings["use_exposure"] else F(1)), branch


def remap(data, mapx, mapy):
    """:413-457"""
    hOrg, wOrg = data.shape
    src = data.ravel()
    xx, yy = mapx.ravel().copy(), mapy.ravel().copy()
    valid = ~(xx < 0)
    xs, ys = np.where(valid, xx, F(0)), np.where(valid, yy, F(0))
    xxi, yyi = xs.astype(np.int32), ys.astype(np.int32)
    xs = xs - xxi.astype(F)
    ys = ys - yyi.astype(F)
    xxyy = xs * ys
    base = xxi.astype(np.int64) + yyi.astype(np.int64) * wOrg
    base = np.where(valid, base, 0)
    with np.errstate(all="ignore"):
        out = xxyy * src[base + 1 + wOrg] + (ys - xxyy) * src[base + wOrg] + (xs - xxyy) * src[base + 1] + (F(1) - xs - ys + xxyy) * src[base]
    return np.where(valid, out, F(0)).astype(F).reshape(mapx.shape)


def undistort(su, ph, raw, exposure, factor=1.0, settings=SETTINGS, mapx=None, mapy=None, passthrough=None):
    """Undistort::undistort<T> for one frame: (plane, exposure_time, branch).  mapx / mapy: a caller's map in place of the set-up's."""
    data, exp, branch = process_frame(raw, ph, exposure, factor, settings)
    pt = su["passthrough"] if passthrough is None else passthrough
    if pt and mapx is None:
        return data.copy(), exp, branch
    return remap(data, su["mapx"] if mapx is None else mapx, su["mapy"] if mapy is None else mapy), exp, branch
