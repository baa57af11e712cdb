"""numpy float32 restatement of DSO's immature points as EDS uses them: FrameHessian::makeImages level 0 (reference
src/tracking/HessianBlocks.cpp:139-202), both ImmaturePoint constructors (src/tracking/ImmaturePoint.cpp:27-114) and
ImmaturePoint::traceOn (:128-467), vectorised over the points of one host frame.  Written from the reference text, independently of
csrc/eds_immature.hpp, with the defined-behaviour rules of include/eds_hip_immature.h: a sample whose 2 x 2 footprint is not wholly inside
the image, or whose coordinate is NaN or beyond +-2^20, is a non-finite hitColor (the reference's own `energy += 1e5` branch); rows 0 and
H - 1 of a frame have gradient 0; a point whose pattern leaves the image is dead.

Every array is float32 and every operation is one IEEE operation on float32 arrays, in the reference's order.  `trace` takes two
switches that are NOT the reference — argmin_le (the arg-min with <= instead of <) and mul_step (ptx = ptx0 + i * dx instead of repeated
addition) — so that the tests can show that their cases tell these apart."""
import numpy as np

F = np.float32
GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
STATUS_NAMES = ("GOOD", "OOB", "OUTLIER", "SKIPPED", "BADCONDITION", "UNINITIALIZED")
PATTERN = ((0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2))      # staticPattern[8], settings.cpp:276

# reference src/utils/settings.cpp:90-165
DEFAULTS = dict(max_pix_search=0.027, trace_stepsize=1.0, trace_gn_iterations=3, trace_gn_threshold=0.1, trace_extra_slack_on_th=1.2,
                trace_slack_interval=1.5, trace_min_improvement_factor=2.0, min_trace_test_radius=2, huber_th=9.0, outlier_th=12.0 * 12.0,
                outlier_th_sum_component=50.0 * 50.0, overall_energy_th_weight=1.0)


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return {k: (int(v) if k in ("trace_gn_iterations", "min_trace_test_radius") else F(v)) for k, v in p.items()}


def same_bits(a, b):
    """elementwise: the same bit pattern, any NaN equal to any NaN (the payload of a NaN an operation makes is not IEEE's to fix)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == np.float32:
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def make_image(color):
    """H x W float32 -> H x W x 3 (colour, dx, dy): the flat-index loop of makeImages, rows 0 and H - 1 with gradient 0"""
    color = np.ascontiguousarray(color, dtype=F)
    H, W = color.shape
    c = color.ravel()
    dx, dy = np.zeros(H * W, F), np.zeros(H * W, F)
    i = np.arange(W, W * (H - 1))
    with np.errstate(all="ignore"):
        gx = F(0.5) * (c[i + 1] - c[i - 1])
        gy = F(0.5) * (c[i + W] - c[i - W])
    dx[i] = np.where(np.isfinite(gx), gx, F(0))
    dy[i] = np.where(np.isfinite(gy), gy, F(0))
    return np.stack([c, dx, dy], axis=1).reshape(H, W, 3)


def _cells(x, y, W, H):
    """the VALID mask of the header's sample rule and the cells (0 where invalid)"""
    with np.errstate(all="ignore"):
        ok = (np.abs(x) <= F(1048576.0)) & (np.abs(y) <= F(1048576.0))
        ix = np.where(ok, x, F(0)).astype(np.int64)           # truncation towards zero, like the C cast
        iy = np.where(ok, y, F(0)).astype(np.int64)
    ok &= (ix >= 0) & (iy >= 0) & (ix <= W - 2) & (iy <= H - 2)
    return ok, np.where(ok, ix, 0), np.where(ok, iy, 0)


def _interp(planes, W, H, x, y):
    """getInterpolatedElement31 / 33 on flat planes; channel 0 is NaN for an invalid sample"""
    ok, ix, iy = _cells(x, y, W, H)
    with np.errstate(all="ignore"):
        dx = x - ix.astype(F)
        dy = y - iy.astype(F)
        dxdy = dx * dy
        w11, w01, w10, w00 = dxdy, dy - dxdy, dx - dxdy, F(1) - dx - dy + dxdy
        o = iy * W + ix
        out = [w11 * p[o + 1 + W] + w01 * p[o + W] + w10 * p[o + 1] + w00 * p[o] for p in planes]
    out[0] = np.where(ok, out[0], F(np.nan))
    return out


def construct(img, uv, typ, idepth=None, distance=None, prm=None):
    """both constructors: idepth and distance None is the first.  Returns the point set as a dict of arrays."""
    prm = prm or params()
    H, W, _ = img.shape
    c = np.ascontiguousarray(img[..., 0]).ravel()
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    n = len(uv)
    color, weights = np.zeros((n, 8), F), np.zeros((n, 8), F)
    g00, g01, g10, g11 = (np.zeros(n, F) for _ in range(4))
    alive = np.ones(n, bool)
    th = prm["outlier_th_sum_component"]
    with np.errstate(all="ignore"):
        for k, (px, py) in enumerate(PATTERN):
            xi, yi = uv[:, 0] + px, uv[:, 1] + py
            x, y = xi.astype(F), yi.astype(F)
            ok, ix, iy = _cells(x, y, W, H)
            o = iy * W + ix
            tl, tr, bl, br = c[o], c[o + 1], c[o + W], c[o + W + 1]
            dx, dy = x - ix.astype(F), y - iy.astype(F)
            top = dx * tr + (F(1) - dx) * tl
            bot = dx * br + (F(1) - dx) * bl
            left = dy * bl + (F(1) - dy) * tl
            right = dy * br + (F(1) - dy) * tr
            col, gx, gy = dx * right + (F(1) - dx) * left, right - left, bot - top
            alive &= ok & np.isfinite(col)
            color[:, k] = col
            g00 = g00 + gx * gx
            g01 = g01 + gx * gy
            g10 = g10 + gy * gx
            g11 = g11 + gy * gy
            weights[:, k] = np.sqrt(th / (th + (gx * gx + gy * gy)))
        e = F(8) * prm["outlier_th"]
        e = e * (prm["overall_energy_th_weight"] * prm["overall_energy_th_weight"])
    P = dict(u=uv[:, 0].astype(F), v=uv[:, 1].astype(F), type=np.asarray(typ, dtype=F).copy(), color=color, weights=weights,
             gradH=np.stack([g00, g01, g10, g11], axis=1), energyTH=np.where(alive, e, F(np.nan)).astype(F), alive=alive,
             idepth_min=np.zeros(n, F), idepth_max=np.full(n, np.nan, F), status=np.full(n, UNINITIALIZED, np.int32),
             quality=np.full(n, 10000.0, F), last_uv=np.zeros((n, 2), F), last_interval=np.zeros(n, F))
    if idepth is not None:
        idepth, distance = np.asarray(idepth, dtype=F), np.asarray(distance, dtype=np.float64)
        seeded = alive & ~(distance > 1.0)
        P["status"][seeded] = GOOD
        P["idepth_min"][seeded] = (idepth.astype(np.float64) - 0.1 * distance).astype(F)[seeded]
        P["idepth_max"][seeded] = (idepth.astype(np.float64) + 0.1 * distance).astype(F)[seeded]
    return P


def copy_points(P):
    return {k: v.copy() for k, v in P.items()}


def summary(P):
    return np.bincount(P["status"][P["alive"]], minlength=6).astype(np.int32)


def trace(P, img, KRKi, Kt, aff, prm=None, argmin_le=False, mul_step=False):
    """traceOn for every live point of P (modified in place) on the frame `img`.  Returns what the branches did, for the tests."""
    prm = prm or params()
    H, W, _ = img.shape
    planes = [np.ascontiguousarray(img[..., k]).ravel() for k in range(3)]
    K = np.asarray(KRKi, dtype=F).reshape(3, 3)
    t = np.asarray(Kt, dtype=F).reshape(3)
    a0, a1 = F(aff[0]), F(aff[1])
    n = len(P["u"])
    u, v = P["u"], P["v"]
    st = dict(n_1e5=0, gn_back=0, gn_break=0, finite_max=0, nonfinite_max=0, horizontal=0, vertical=0, outlier_twice=0, max_steps=[])

    def leave(mask, status, uu=None, vv=None, interval=None):
        P["status"][mask] = status if np.isscalar(status) else status[mask]
        P["last_uv"][mask, 0] = F(-1) if uu is None else uu[mask]
        P["last_uv"][mask, 1] = F(-1) if vv is None else vv[mask]
        P["last_interval"][mask] = F(0) if interval is None else interval[mask]

    def inside(uu, vv):
        return (uu > 4) & (vv > 4) & (uu < W - 5) & (vv < H - 5)

    with np.errstate(all="ignore"):
        todo = P["alive"] & (P["status"] != OOB)
        max_pix = F(W + H) * prm["max_pix_search"]
        pr = [K[i, 0] * u + K[i, 1] * v + K[i, 2] * F(1) for i in range(3)]
        idmin, idmax = P["idepth_min"].copy(), P["idepth_max"].copy()
        pmin = [pr[i] + t[i] * idmin for i in range(3)]
        uMin, vMin = pmin[0] / pmin[2], pmin[1] / pmin[2]
        m = todo & ~inside(uMin, vMin)
        leave(m, OOB)
        todo &= ~m

        fin = np.isfinite(idmax)
        st["finite_max"], st["nonfinite_max"] = int((todo & fin).sum()), int((todo & ~fin).sum())
        # idepth_max finite: project it
        pmax = [pr[i] + t[i] * idmax for i in range(3)]
        uA, vA = pmax[0] / pmax[2], pmax[1] / pmax[2]
        distA = np.sqrt((uMin - uA) * (uMin - uA) + (vMin - vA) * (vMin - vA))
        # not finite: an arbitrary depth gives the direction
        parb = [pr[i] + t[i] * F(0.01) for i in range(3)]
        ex, ey = parb[0] / parb[2] - uMin, parb[1] / parb[2] - vMin
        d = F(1) / np.sqrt(ex * ex + ey * ey)
        uB, vB = uMin + max_pix * ex * d, vMin + max_pix * ey * d
        uMax, vMax = np.where(fin, uA, uB), np.where(fin, vA, vB)
        dist = np.where(fin, distA, max_pix).astype(F)
        m = todo & ~inside(uMax, vMax)
        leave(m, OOB)
        todo &= ~m
        m = todo & fin & (dist < prm["trace_slack_interval"])
        leave(m, SKIPPED, (uMax + uMin) * F(0.5), (vMax + vMin) * F(0.5), dist)
        todo &= ~m
        m = todo & ~((idmin < 0) | ((pmin[2] > F(0.75)) & (pmin[2] < F(1.5))))
        leave(m, OOB)
        todo &= ~m

        dx = prm["trace_stepsize"] * (uMax - uMin)
        dy = prm["trace_stepsize"] * (vMax - vMin)
        G = P["gradH"]
        qa = (dx * G[:, 0] + dy * G[:, 2]) * dx + (dx * G[:, 1] + dy * G[:, 3]) * dy
        ndx = -dx
        qb = (dy * G[:, 0] + ndx * G[:, 2]) * dy + (dy * G[:, 1] + ndx * G[:, 3]) * ndx
        eip = F(0.2) + F(0.2) * (qa + qb) / qa
        m = todo & (eip * prm["trace_min_improvement_factor"] > dist) & fin
        leave(m, BADCONDITION, (uMax + uMin) * F(0.5), (vMax + vMin) * F(0.5), dist)
        todo &= ~m
        eip = np.where(eip > 10, F(10), eip).astype(F)

        dx = dx / dist
        dy = dy / dist
        dist = np.where(dist > max_pix, max_pix, dist).astype(F)
        nf = F(1.9999) + dist / prm["trace_stepsize"]
        steps = np.where(nf < F(100), np.where(nf < F(100), nf, F(0)).astype(np.int64), 99)
        steps = np.where(steps >= 100, 99, steps)
        shift = uMin * F(1000) - np.floor(uMin * F(1000))
        x0, y0 = uMin - shift * dx, vMin - shift * dy
        rot = [(K[0, 0] * F(px) + K[0, 1] * F(py), K[1, 0] * F(px) + K[1, 1] * F(py)) for px, py in PATTERN]
        m = todo & ~(np.isfinite(dx) & np.isfinite(dy))
        leave(m, OOB)
        todo &= ~m
        st["max_steps"] = sorted(set(steps[todo].tolist()))

        # the discrete search
        errors = np.full((n, 99), np.nan, F)
        bestU, bestV, bestE = np.zeros(n, F), np.zeros(n, F), np.full(n, 1e10, F)
        bestI = np.full(n, -1, np.int64)
        x, y = x0.copy(), y0.copy()
        target_col = [a0 * P["color"][:, k] + a1 for k in range(8)]
        hub = prm["huber_th"]
        for i in range(int(steps[todo].max()) if todo.any() else 0):
            act = todo & (i < steps)
            if mul_step:
                x, y = x0 + F(i) * dx, y0 + F(i) * dy
            energy = np.zeros(n, F)
            for k in range(8):
                hit = _interp(planes[:1], W, H, x + rot[k][0], y + rot[k][1])[0]
                bad = ~np.isfinite(hit)
                r = hit - target_col[k]
                hw = np.where(np.abs(r) < hub, F(1), hub / np.abs(r)).astype(F)
                energy = np.where(bad, energy + F(1e5), energy + hw * r * r * (F(2) - hw)).astype(F)
                st["n_1e5"] += int((bad & act).sum())
            errors[act, i] = energy[act]
            better = act & ((energy <= bestE) if argmin_le else (energy < bestE))
            bestU, bestV = np.where(better, x, bestU), np.where(better, y, bestV)
            bestE, bestI = np.where(better, energy, bestE), np.where(better, i, bestI)
            if not mul_step:
                x, y = x + dx, y + dy
        second = np.full(n, 1e10, F)
        rad = prm["min_trace_test_radius"]
        for i in range(int(steps[todo].max()) if todo.any() else 0):
            m = todo & (i < steps) & ((i < bestI - rad) | (i > bestI + rad)) & (errors[:, i] < second)
            second = np.where(m, errors[:, i], second)
        newq = second / bestE
        m = todo & ((newq < P["quality"]) | (steps > 10))
        P["quality"][m] = newq[m]

        # Gauss-Newton on the line
        uBak, vBak = bestU.copy(), bestV.copy()
        back = np.zeros(n, F)
        if prm["trace_gn_iterations"] > 0:
            bestE = np.full(n, 1e5, F)
        run = todo.copy()
        w2 = P["weights"] * P["weights"]
        for _ in range(prm["trace_gn_iterations"]):
            Hs, b, energy = np.ones(n, F), np.zeros(n, F), np.zeros(n, F)
            for k in range(8):
                hc, hx, hy = _interp(planes, W, H, bestU + rot[k][0], bestV + rot[k][1])
                bad = ~np.isfinite(hc)
                r = hc - target_col[k]
                dres = dx * hx + dy * hy
                hw = np.where(np.abs(r) < hub, F(1), hub / np.abs(r)).astype(F)
                Hs = np.where(bad, Hs, Hs + hw * dres * dres)
                b = np.where(bad, b, b + hw * r * dres)
                energy = np.where(bad, energy + F(1e5), energy + w2[:, k] * hw * r * r * (F(2) - hw)).astype(F)
                st["n_1e5"] += int((bad & run).sum())
            worse = run & (energy > bestE)
            good = run & ~worse
            st["gn_back"] += int(worse.sum())
            back = np.where(worse, back * F(0.5), back)
            step = -F(1) * b / Hs
            step = np.where(step < F(-0.5), F(-0.5), np.where(step > F(0.5), F(0.5), step))
            step = np.where(np.isfinite(step), step, F(0)).astype(F)
            uBak, vBak = np.where(good, bestU, uBak), np.where(good, bestV, vBak)
            back = np.where(good, step, back).astype(F)
            bestU = np.where(worse, uBak + back * dx, np.where(good, bestU + step * dx, bestU)).astype(F)
            bestV = np.where(worse, vBak + back * dy, np.where(good, bestV + step * dy, bestV)).astype(F)
            bestE = np.where(good, energy, bestE)
            brk = run & (np.abs(back) < prm["trace_gn_threshold"])
            st["gn_break"] += int(brk.sum())
            run &= ~brk

        # the energy-based outlier test; a second OUTLIER in a row is OOB
        m = todo & ~(bestE < P["energyTH"] * prm["trace_extra_slack_on_th"])
        again = m & (P["status"] == OUTLIER)
        st["outlier_twice"] = int(again.sum())
        leave(m, np.where(again, OOB, OUTLIER).astype(np.int32))
        todo &= ~m

        # the new interval
        hor = dx * dx > dy * dy
        st["horizontal"], st["vertical"] = int((todo & hor).sum()), int((todo & ~hor).sum())
        lo = np.where(hor, (pr[2] * (bestU - eip * dx) - pr[0]) / (t[0] - t[2] * (bestU - eip * dx)),
                      (pr[2] * (bestV - eip * dy) - pr[1]) / (t[1] - t[2] * (bestV - eip * dy))).astype(F)
        hi = np.where(hor, (pr[2] * (bestU + eip * dx) - pr[0]) / (t[0] - t[2] * (bestU + eip * dx)),
                      (pr[2] * (bestV + eip * dy) - pr[1]) / (t[1] - t[2] * (bestV + eip * dy))).astype(F)
        swap = lo > hi
        lo, hi = np.where(swap, hi, lo), np.where(swap, lo, hi)
        P["idepth_min"][todo] = lo[todo]
        P["idepth_max"][todo] = hi[todo]
        m = todo & (~np.isfinite(lo) | ~np.isfinite(hi) | (hi < 0))
        leave(m, OUTLIER)
        todo &= ~m
        leave(todo, GOOD, bestU, bestV, F(2) * eip)
    return st
