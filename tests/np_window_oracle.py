"""A numpy oracle of the per-residual and per-point part of DSO's window optimiser, written from the reference text
(src/tracking/Residuals.cpp:69-320, src/tracking/ResidualProjections.h:46-86, src/bundles/EnergyFunctionalStructs.cpp:38-48,
src/bundles/AccumulatedTopHessian.cpp:49-145, src/bundles/AccumulatedSCHessian.cpp:36-55), independent of csrc/eds_window.hpp: float32 per
residual in the reference's operand order, vectorised over the residuals with the taps and a point's residuals walked in order; the
energy summed EXACTLY (math.fsum).  Every decisive comparison records its margin, so a case can show that no residual is undecided.
The keyword switches of ``Oracle`` (fy_is_fx, swap_jabjidx, no_sqrt, reverse_taps) exist only for tests/test_window_oracle.py, which
shows that the cases tell these variants apart."""
import math

import numpy as np

from np_coarse_oracle import make_images, same_bits  # noqa: F401  (level 0 of makeImages is the coarse oracle's)

f32 = np.float32
IN, OOB, OUTLIER = 0, 1, 2
PATTERN = ((0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2))        # staticPattern[8] (settings.cpp)
# settings.cpp:91-127 and HessianBlocks.h:58-62
DEFAULTS = dict(outlier_th_sum_component=50.0 * 50.0, huber_th=9.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8, scale_idepth=1.0,
                scale_f=1.0, scale_c=1.0)
J_RESF, J_JPDXI, J_JPDC, J_JPDD, J_JIDX, J_JABF, J_JIDX2, J_JABJIDX, J_JAB2, J_WORDS = 0, 8, 20, 28, 30, 46, 62, 66, 70, 74
UNDECIDED_ULPS = 4


def params(**over):
    p = {k: f32(v) for k, v in DEFAULTS.items()}
    p.update({k: f32(v) for k, v in over.items()})
    return p


def _margin(a, b):
    """how many ulps of the larger side separate the two sides of a comparison (inf where either is not finite: such a comparison is
    decided by the NaN rule, not by rounding)"""
    with np.errstate(all="ignore"):
        a, b = np.asarray(a, f32), np.broadcast_to(np.asarray(b, f32), np.shape(a))
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32)).astype(np.float64)
        return np.where(np.isfinite(a) & np.isfinite(b), d, np.inf)


class Oracle:
    def __init__(self, H, W, K, prm=None, fy_is_fx=False, swap_jabjidx=False, no_sqrt=False, reverse_taps=False):
        self.H, self.W = H, W
        self.s = params(**(prm or {}))
        fx, fy, cx, cy = (f32(v) for v in K)
        if fy_is_fx:
            fy = fx
        self.fx, self.fy, self.cx, self.cy, self.fxi, self.fyi = fx, fy, cx, cy, f32(1) / fx, f32(1) / fy
        self.wM3, self.hM3 = f32(W - 3), f32(H - 3)
        self.swap_jabjidx, self.no_sqrt, self.reverse_taps = swap_jabjidx, no_sqrt, reverse_taps
        self.frames = {}
        self.n = self.m = 0

    def set_frames(self, first, images):
        images = np.asarray(images, f32)
        for k, img in enumerate(images[None] if images.ndim == 2 else images):
            self.frames[first + k] = make_images(img, 1)[0].reshape(-1, 3)

    def frame(self, f):
        return self.frames[f].reshape(self.H, self.W, 3)

    def set_points(self, host, uv, color, weights, idepth_scaled, idepth_zero_scaled=None):
        self.host = np.asarray(host, np.int32)
        self.n = len(self.host)
        self.uv, self.color, self.weights = np.asarray(uv, f32).reshape(-1, 2), np.asarray(color, f32).reshape(-1, 8), np.asarray(weights, f32).reshape(-1, 8)
        self.ids = np.asarray(idepth_scaled, f32).copy()
        self.idz = self.ids.copy() if idepth_zero_scaled is None else np.asarray(idepth_zero_scaled, f32).copy()
        self.set_residuals([], [])

    def set_idepths(self, idepth_scaled=None, idepth_zero_scaled=None):
        if idepth_scaled is not None:
            self.ids = np.asarray(idepth_scaled, f32).copy()
        if idepth_zero_scaled is not None:
            self.idz = np.asarray(idepth_zero_scaled, f32).copy()

    def set_residuals(self, point, target, state=None, energy=None):
        self.point, self.target = np.asarray(point, np.int64), np.asarray(target, np.int64)
        m = self.m = len(self.point)
        self.r = dict(state=np.zeros(m, np.int32) if state is None else np.asarray(state, np.int32).copy(),
                      energy=np.zeros(m, f32) if energy is None else np.asarray(energy, f32).copy(),
                      new_state=np.full(m, OUTLIER, np.int32), new_energy_with_outlier=np.zeros(m, f32), linearize_return=np.zeros(m, f32),
                      is_active=np.zeros(m, np.int32), center_projected_to=np.zeros((m, 3), f32), projected_to=np.zeros((m, 8, 2), f32),
                      J=np.zeros((m, J_WORDS), f32), ef_J=np.zeros((m, J_WORDS), f32), JpJdF=np.zeros((m, 8), f32))
        self.r["new_energy"] = self.r["energy"].copy()
        self.res_first = np.concatenate([[0], np.cumsum(np.bincount(self.point, minlength=self.n))]).astype(np.int64)

    # ---- Residuals.cpp:69-265 ----------------------------------------------------------------------------------------------------------
    def linearize(self, F, precalc, frame_energy_th):
        """returns dict(energy exact, abs = sum |return|, counts, undecided)"""
        s, r, m = self.s, self.r, self.m
        th = np.asarray(frame_energy_th, f32)
        if m == 0:
            return dict(energy=0.0, abs=0.0, counts=np.zeros(3, np.int32), undecided=0)
        host = self.host[self.point]
        pc = np.asarray(precalc, f32).reshape(F * F, 27)[host * F + self.target]
        KRKi, Kt, R, t, aff, b0 = pc[:, 0:9], pc[:, 9:12], pc[:, 12:21], pc[:, 21:24], pc[:, 24:26], pc[:, 26]
        u_pt, v_pt = self.uv[self.point, 0], self.uv[self.point, 1]
        ids, idz = self.ids[self.point], self.idz[self.point]
        fx, fy, cx, cy, fxi, fyi = self.fx, self.fy, self.cx, self.cy, self.fxi, self.fyi
        one = f32(1)
        close = np.zeros(m, bool)                                    # a decisive comparison within UNDECIDED_ULPS of flipping
        with np.errstate(all="ignore"):
            r["new_energy_with_outlier"][:] = -1
            live = r["state"] != OOB
            # projectPoint, the long overload (ResidualProjections.h:60-86)
            k0, k1 = ((u_pt + f32(0)) - cx) * fxi, ((v_pt + f32(0)) - cy) * fyi
            p0 = ((R[:, 0] * k0 + R[:, 1] * k1) + R[:, 2] * one) + t[:, 0] * idz
            p1 = ((R[:, 3] * k0 + R[:, 4] * k1) + R[:, 5] * one) + t[:, 1] * idz
            p2 = ((R[:, 6] * k0 + R[:, 7] * k1) + R[:, 8] * one) + t[:, 2] * idz
            drescale = one / p2
            new_idepth = idz * drescale
            u, v = p0 * drescale, p1 * drescale
            Ku, Kv = u * fx + cx, v * fy + cy
            pos = drescale > 0
            inb = (Ku > f32(1.1)) & (Kv > f32(1.1)) & (Ku < self.wM3) & (Kv < self.hM3)
            centre = live & pos & inb
            edge = np.minimum(np.minimum(_margin(Ku, f32(1.1)), _margin(Kv, f32(1.1))), np.minimum(_margin(Ku, self.wM3), _margin(Kv, self.hM3)))
            close |= live & pos & (edge <= UNDECIDED_ULPS)
            r["center_projected_to"][centre] = np.stack([Ku, Kv, new_idepth], axis=1)[centre]
            d_d_x = ((drescale * (t[:, 0] - t[:, 2] * u)) * s["scale_idepth"]) * fx
            d_d_y = ((drescale * (t[:, 1] - t[:, 2] * v)) * s["scale_idepth"]) * fy
            cx2 = drescale * (R[:, 6] * u - R[:, 0])
            cx3 = ((fx * drescale) * (R[:, 7] * u - R[:, 1])) * fyi
            cx0, cx1 = k0 * cx2, k1 * cx3
            cy2 = ((fy * drescale) * (R[:, 6] * v - R[:, 3])) * fxi
            cy3 = drescale * (R[:, 7] * v - R[:, 4])
            cy0, cy1 = k0 * cy2, k1 * cy3
            Jpdc = np.stack([(cx0 + u) * s["scale_f"], cx1 * s["scale_f"], (cx2 + one) * s["scale_c"], cx3 * s["scale_c"],
                             cy0 * s["scale_f"], (cy1 + v) * s["scale_f"], cy2 * s["scale_c"], (cy3 + one) * s["scale_c"]], axis=1)
            z = np.zeros(m, f32)
            Jpdxi = np.stack([new_idepth * fx, z, (-new_idepth * u) * fx, (-u * v) * fx, (one + u * u) * fx, (-v) * fx,
                              z, new_idepth * fy, (-new_idepth * v) * fy, (-(one + v * v)) * fy, (u * v) * fy, u * fy], axis=1)

            # the pattern loop (:174-236)
            alive = centre.copy()                                    # has not returned OOB yet
            taps, nonfinite, huber = [], 0, [0, 0]
            for idx, (px, py) in enumerate(PATTERN):
                x, y = u_pt + f32(px), v_pt + f32(py)
                q0 = ((KRKi[:, 0] * x + KRKi[:, 1] * y) + KRKi[:, 2] * one) + Kt[:, 0] * ids
                q1 = ((KRKi[:, 3] * x + KRKi[:, 4] * y) + KRKi[:, 5] * one) + Kt[:, 1] * ids
                q2 = ((KRKi[:, 6] * x + KRKi[:, 7] * y) + KRKi[:, 8] * one) + Kt[:, 2] * ids
                tKu, tKv = q0 / q2, q1 / q2
                ok = (tKu > f32(1.1)) & (tKv > f32(1.1)) & (tKu < self.wM3) & (tKv < self.hM3)
                edge = np.minimum(np.minimum(_margin(tKu, f32(1.1)), _margin(tKv, f32(1.1))), np.minimum(_margin(tKu, self.wM3), _margin(tKv, self.hM3)))
                close |= alive & (edge <= UNDECIDED_ULPS)
                alive &= ok
                r["projected_to"][alive, idx, 0], r["projected_to"][alive, idx, 1] = tKu[alive], tKv[alive]
                sx, sy = np.where(alive, tKu, f32(2)), np.where(alive, tKv, f32(2))
                ix, iy = sx.astype(np.int32), sy.astype(np.int32)
                dx, dy = sx - ix.astype(f32), sy - iy.astype(f32)
                dxdy = dx * dy
                hit = np.zeros((m, 3), f32)
                for tg in np.unique(self.target):
                    sel = self.target == tg
                    img, b = self.frames[int(tg)], ix[sel] + iy[sel] * self.W
                    w11, w01, w10, w00 = dxdy[sel, None], (dy - dxdy)[sel, None], (dx - dxdy)[sel, None], (one - dx - dy + dxdy)[sel, None]
                    hit[sel] = w11 * img[b + 1 + self.W] + w01 * img[b + self.W] + w10 * img[b + 1] + w00 * img[b]
                col, wgt = self.color[self.point, idx], self.weights[self.point, idx]
                residual = hit[:, 0] - (aff[:, 0] * col + aff[:, 1])
                drdA = col - b0
                nonfinite += int((alive & ~np.isfinite(hit[:, 0])).sum())
                alive &= np.isfinite(hit[:, 0])
                c = s["outlier_th_sum_component"]
                w = np.sqrt(c / (c + (hit[:, 1] * hit[:, 1] + hit[:, 2] * hit[:, 2])))
                w = f32(0.5) * (w + wgt)
                ar = np.abs(residual)
                close |= alive & (_margin(ar, s["huber_th"]) <= UNDECIDED_ULPS)
                hw = np.where(ar < s["huber_th"], one, s["huber_th"] / ar)
                huber[0] += int((alive & (ar < s["huber_th"])).sum())
                huber[1] += int((alive & ~(ar < s["huber_th"])).sum())
                e = w * w * hw * residual * residual * (f32(2) - hw)
                if not self.no_sqrt:
                    hw = np.where(hw < 1, np.sqrt(hw), hw)
                hw = hw * w
                h1, h2 = hit[:, 1] * hw, hit[:, 2] * hw
                ja, jb = drdA * hw, hw
                prods = [h1 * h1, h2 * h2, h1 * h2, drdA * hw * h1, drdA * hw * h2, hw * h1, hw * h2, drdA * drdA * hw * hw, drdA * hw * hw, hw * hw]
                wji2 = hw * hw * (h1 * h1 + h2 * h2)
                if s["affine_opt_mode_a"] < 0:
                    ja = np.zeros(m, f32)
                if s["affine_opt_mode_b"] < 0:
                    jb = np.zeros(m, f32)
                taps.append(dict(resF=residual * hw, jx=h1, jy=h2, ja=ja, jb=jb, e=e, wji2=wji2, prods=prods))
            order = range(7, -1, -1) if self.reverse_taps else range(8)
            energy_left, wji2_sum, sums = np.zeros(m, f32), np.zeros(m, f32), [np.zeros(m, f32) for _ in range(10)]
            for idx in order:
                energy_left = energy_left + taps[idx]["e"]
                wji2_sum = wji2_sum + taps[idx]["wji2"]
                sums = [a + b for a, b in zip(sums, taps[idx]["prods"])]
            J = np.zeros((m, J_WORDS), f32)
            for idx in range(8):
                tp = taps[idx]
                J[:, J_RESF + idx], J[:, J_JIDX + idx], J[:, J_JIDX + 8 + idx] = tp["resF"], tp["jx"], tp["jy"]
                J[:, J_JABF + idx], J[:, J_JABF + 8 + idx] = tp["ja"], tp["jb"]
            J[:, J_JPDXI:J_JPDXI + 12], J[:, J_JPDC:J_JPDC + 8] = Jpdxi, Jpdc
            J[:, J_JPDD], J[:, J_JPDD + 1] = d_d_x, d_d_y
            for k, q in enumerate((0, 2, 2, 1)):
                J[:, J_JIDX2 + k] = sums[q]
            for k, q in enumerate((3, 5, 4, 6) if self.swap_jabjidx else (3, 4, 5, 6)):
                J[:, J_JABJIDX + k] = sums[q]
            for k, q in enumerate((7, 8, 8, 9)):
                J[:, J_JAB2 + k] = sums[q]
            th_max = np.where(th[host] < th[self.target], th[self.target], th[host])
            outlier = (energy_left > th_max) | (wji2_sum < 2)
            close |= alive & ((_margin(energy_left, th_max) <= UNDECIDED_ULPS) | (_margin(wji2_sum, f32(2)) <= UNDECIDED_ULPS))
            # an OOB linearize leaves J, state_NewEnergy and the return value's source as they were
            r["J"][alive] = J[alive]
            r["new_energy_with_outlier"][alive] = energy_left[alive]
            r["new_state"][:] = np.where(alive, np.where(outlier, OUTLIER, IN), OOB)
            r["new_energy"][alive] = np.where(outlier, th_max, energy_left)[alive]
            r["linearize_return"][:] = np.where(alive, r["new_energy"], r["energy"])
        ret = r["linearize_return"].astype(np.float64)
        self.margins = dict(outlier_by_energy=int((alive & (energy_left > th_max)).sum()), outlier_by_gradient=int((alive & ~(energy_left > th_max) & (wji2_sum < 2)).sum()),
                            oob_entry=int((~live).sum()), oob_drescale=int((live & ~pos).sum()), oob_centre=int((live & pos & ~inb).sum()),
                            oob_taps=int((centre & ~alive).sum()), oob_nonfinite=nonfinite, huber_quadratic=huber[0], huber_linear=huber[1],
                            new_in=int((alive & ~outlier).sum()))
        return dict(energy=math.fsum(ret), abs=math.fsum(np.abs(ret)), counts=np.bincount(r["new_state"], minlength=3).astype(np.int32),
                    undecided=int(close.sum()))

    # ---- Residuals.cpp:298-320, EnergyFunctionalStructs.cpp:38-48 ------------------------------------------------------------------------
    def apply(self, copy_jacobians=True):
        r = self.r
        if self.m == 0:
            return
        stay = np.zeros(self.m, bool)
        if copy_jacobians:
            stay = r["state"] == OOB
            take = ~stay & (r["new_state"] == IN)
            r["is_active"][~stay] = take[~stay]
            r["ef_J"][take] = r["J"][take]
            J = r["ef_J"][take]
            d0, d1 = J[:, J_JPDD], J[:, J_JPDD + 1]
            a = J[:, J_JIDX2] * d0 + J[:, J_JIDX2 + 1] * d1
            b = J[:, J_JIDX2 + 2] * d0 + J[:, J_JIDX2 + 3] * d1
            out = np.zeros((len(J), 8), f32)
            for i in range(6):
                out[:, i] = J[:, J_JPDXI + i] * a + J[:, J_JPDXI + 6 + i] * b
            out[:, 6] = J[:, J_JABJIDX] * d0 + J[:, J_JABJIDX + 1] * d1
            out[:, 7] = J[:, J_JABJIDX + 2] * d0 + J[:, J_JABJIDX + 3] * d1
            r["JpJdF"][take] = out
        r["state"][~stay] = r["new_state"][~stay]
        r["energy"][~stay] = r["new_energy"][~stay]

    # ---- AccumulatedTopHessian.cpp:49-145 (mode 0, per point) and AccumulatedSCHessian.cpp:36-55 --------------------------------------------
    def point_hessians(self, priorF=None, deltaF=None, lf=None, shift_prior_to_zero=False):
        n, r = self.n, self.r
        prior = np.zeros(n, f32) if priorF is None else np.asarray(priorF, f32)
        delta = np.zeros(n, f32) if deltaF is None else np.asarray(deltaF, f32)
        lf = np.zeros((n, 6), f32) if lf is None else np.asarray(lf, f32).reshape(n, 6)
        bd, Hdd, Hcd, cnt = np.zeros(n, f32), np.zeros(n, f32), np.zeros((n, 4), f32), np.zeros(n, np.int32)
        per = np.diff(self.res_first)
        with np.errstate(all="ignore"):
            for k in range(int(per.max()) if n and self.m else 0):
                pts = np.nonzero(per > k)[0]
                ri = self.res_first[pts] + k
                on = r["is_active"][ri] != 0
                pts, ri = pts[on], ri[on]
                J = r["ef_J"][ri]
                jr0, jr1 = np.zeros(len(ri), f32), np.zeros(len(ri), f32)
                for i in range(8):
                    jr0 = jr0 + J[:, J_RESF + i] * J[:, J_JIDX + i]
                    jr1 = jr1 + J[:, J_RESF + i] * J[:, J_JIDX + 8 + i]
                d0, d1 = J[:, J_JPDD], J[:, J_JPDD + 1]
                q0 = J[:, J_JIDX2] * d0 + J[:, J_JIDX2 + 1] * d1
                q1 = J[:, J_JIDX2 + 2] * d0 + J[:, J_JIDX2 + 3] * d1
                bd[pts] = bd[pts] + (jr0 * d0 + jr1 * d1)
                Hdd[pts] = Hdd[pts] + (q0 * d0 + q1 * d1)
                Hcd[pts] = Hcd[pts] + (J[:, J_JPDC:J_JPDC + 4] * q0[:, None] + J[:, J_JPDC + 4:J_JPDC + 8] * q1[:, None])
                cnt[pts] += 1
            H = Hdd + lf[:, 0] + prior
            H = np.where(H.astype(np.float64) < 1e-10, f32(1e-10), H)
            HdiF = (1.0 / H.astype(np.float64)).astype(f32)
            bdSum = bd + lf[:, 1]
            if shift_prior_to_zero:
                bdSum = bdSum + prior * delta
        none = cnt == 0
        self.p = dict(Hdd_accAF=Hdd, bd_accAF=bd, Hcd_accAF=Hcd, HdiF=np.where(none, f32(0), HdiF), bdSumF=np.where(none, f32(0), bdSum).astype(f32),
                      idepth_hessian=np.where(none, f32(0), H).astype(f32), nres=cnt)
        self.clamped = int((~none & ((Hdd + lf[:, 0] + prior).astype(np.float64) < 1e-10)).sum())
        return int(cnt.sum())

    def residuals(self):
        return {k: v.copy() for k, v in self.r.items()}

    def points(self):
        return {k: v.copy() for k, v in self.p.items()}


# ---- the accumulators (AccumulatedTopHessian.cpp:115-129, MatrixAccumulators.h:754-915, AccumulatedSCHessian.cpp:56-76) and stitches ----------
TOP_WORDS, E_WORDS, D_WORDS, C_WORDS = 92, 40, 65, 20


def acc_offsets(F):
    e = F * F * TOP_WORDS
    d = e + F * F * E_WORDS
    c = d + F * F * F * D_WORDS
    return e, d, c, c + F * C_WORDS


def top_terms(J):
    """the 91 fp32 addends of every row of J (k x 74) to its acc[h + F t], in the reference's operand order"""
    x = np.concatenate([J[:, J_JPDC:J_JPDC + 4], J[:, J_JPDXI:J_JPDXI + 6]], axis=1)
    y = np.concatenate([J[:, J_JPDC + 4:J_JPDC + 8], J[:, J_JPDXI + 6:J_JPDXI + 12]], axis=1)
    a, b, c = J[:, J_JIDX2], J[:, J_JIDX2 + 1], J[:, J_JIDX2 + 3]
    out = []
    for col in range(10):
        for row in range(col, 10):
            out.append(a * x[:, row] * x[:, col] + c * y[:, row] * y[:, col] + b * (x[:, row] * y[:, col] + y[:, row] * x[:, col]))
    res = J[:, J_RESF:J_RESF + 8]

    def dot(u, v):
        s = np.zeros(len(J), f32)
        for i in range(8):
            s = s + u[:, i] * v[:, i]
        return s
    ji0, ji1 = dot(res, J[:, J_JIDX:J_JIDX + 8]), dot(res, J[:, J_JIDX + 8:J_JIDX + 16])
    ja0, ja1 = dot(res, J[:, J_JABF:J_JABF + 8]), dot(res, J[:, J_JABF + 8:J_JABF + 16])
    tr = ((J[:, J_JABJIDX], J[:, J_JABJIDX + 1]), (J[:, J_JABJIDX + 2], J[:, J_JABJIDX + 3]), (ji0, ji1))
    for k in range(10):
        for q in range(3):
            out.append(x[:, k] * tr[q][0] + y[:, k] * tr[q][1])
    out += [J[:, J_JAB2], J[:, J_JAB2 + 1], ja0, J[:, J_JAB2 + 3], ja1, dot(res, res)]
    return np.stack(out, axis=1).astype(f32)


def accumulate(o, F, lf=None, swap_index=False):
    """exact accumulators (math.fsum of the fp32 terms) in the flat layout of csrc/eds_window.hpp, and per word the derived bound
    n 2^-53 sum|term| with n the points of the word's host frame; swap_index: h F + t for h + F t (a mutation)"""
    off_e, off_d, off_c, size = acc_offsets(F)
    terms = [[] for _ in range(size)]
    idx = (lambda h, t: h * F + t) if swap_index else (lambda h, t: h + F * t)
    r, p = o.r, o.p
    lf = np.zeros((o.n, 6), f32) if lf is None else np.asarray(lf, f32).reshape(o.n, 6)
    act = np.nonzero(r["is_active"])[0]
    T = top_terms(r["ef_J"][act])
    host = o.host[o.point]
    for k, ri in enumerate(act):
        base = idx(int(host[ri]), int(o.target[ri])) * TOP_WORDS
        for e in range(91):
            terms[base + e].append(float(T[k, e]))
        terms[base + 91].append(1.0)
    Hcd = (p["Hcd_accAF"] + lf[:, 2:6]).astype(f32)
    for pt in range(o.n):
        if p["nres"][pt] == 0:
            continue
        h, hdi, bds, hc = int(o.host[pt]), p["HdiF"][pt], p["bdSumF"][pt], Hcd[pt]
        base = off_c + h * C_WORDS
        for i in range(4):
            for j in range(4):
                terms[base + 4 * i + j].append(float((hdi * hc[i]) * hc[j]))
            terms[base + 16 + i].append(float((bds * hdi) * hc[i]))
        rs = [ri for ri in range(o.res_first[pt], o.res_first[pt + 1]) if r["is_active"][ri]]
        for r1 in rs:
            a1, J1 = idx(h, int(o.target[r1])), r["JpJdF"][r1]
            for r2 in rs:
                J2 = r["JpJdF"][r2]
                base = off_d + (a1 + int(o.target[r2]) * F * F) * D_WORDS
                blk = np.outer(hdi * J1, J2).astype(f32)             # (w L[i]) R[j]
                for e in range(64):
                    terms[base + e].append(float(blk[e // 8, e % 8]))
                terms[base + 64].append(1.0)
            base = off_e + a1 * E_WORDS
            blk = np.outer(hdi * J1, hc).astype(f32)
            for e in range(32):
                terms[base + e].append(float(blk[e // 4, e % 4]))
            w = f32(hdi * bds)
            for i in range(8):
                terms[base + 32 + i].append(float(w * J1[i]))
    counts = np.bincount(o.host, minlength=F).astype(np.float64)
    n_of = np.empty(size)                                        # the points of the word's own host frame: the additions of its fold
    n_of[:off_e] = counts[(np.arange(off_e) // TOP_WORDS) % F]
    n_of[off_e:off_d] = counts[(np.arange(off_d - off_e) // E_WORDS) % F]
    n_of[off_d:off_c] = counts[(np.arange(off_c - off_d) // D_WORDS) % F]
    n_of[off_c:] = counts[np.arange(size - off_c) // C_WORDS]
    if swap_index:
        n_of[:] = counts.max()
    acc = np.array([math.fsum(t) for t in terms])
    absum = np.array([math.fsum(abs(v) for v in t) for t in terms])
    return acc, absum * n_of * 2.0 ** -53


def stitch(F, acc, adH, adT):
    """stitchDouble(usePrior = false) and the Schur stitch (AccumulatedTopHessian.cpp:171-225, AccumulatedSCHessian.cpp:159-219), numpy matmul"""
    off_e, off_d, off_c, _ = acc_offsets(F)
    N = 4 + 8 * F
    HA, bA, Hs, bs = np.zeros((N, N)), np.zeros(N), np.zeros((N, N)), np.zeros(N)
    for h in range(F):
        for t in range(F):
            a = h + F * t
            w = acc[a * TOP_WORDS:(a + 1) * TOP_WORDS]
            if w[91] == 0:
                continue
            H = np.zeros((13, 13))
            iu = [(r, c) for r in range(10) for c in range(r, 10)]
            for k, (r, c) in enumerate(iu):
                H[r, c] = H[c, r] = w[k]
            H[:10, 10:] = w[55:85].reshape(10, 3)
            H[10:, :10] = H[:10, 10:].T
            H[10, 10], H[10, 11], H[10, 12], H[11, 11], H[11, 12], H[12, 12] = w[85:91]
            H[11, 10], H[12, 10], H[12, 11] = H[10, 11], H[10, 12], H[11, 12]
            hs, ts = slice(4 + 8 * h, 12 + 8 * h), slice(4 + 8 * t, 12 + 8 * t)
            M = H[4:12, 4:12]
            HA[hs, hs] += adH[a] @ M @ adH[a].T
            HA[ts, ts] += adT[a] @ M @ adT[a].T
            HA[hs, ts] += adH[a] @ M @ adT[a].T
            HA[hs, :4] += adH[a] @ H[4:12, :4]
            HA[ts, :4] += adT[a] @ H[4:12, :4]
            HA[:4, :4] += H[:4, :4]
            bA[hs] += adH[a] @ H[4:12, 12]
            bA[ts] += adT[a] @ H[4:12, 12]
            bA[:4] += H[:4, 12]
    for h in range(F):
        hs = slice(4 + 8 * h, 12 + 8 * h)
        HA[:4, hs] = HA[hs, :4].T
        for t in range(h + 1, F):
            ts = slice(4 + 8 * t, 12 + 8 * t)
            HA[hs, ts] += HA[ts, hs].T
            HA[ts, hs] = HA[hs, ts].T
    for i in range(F):
        for j in range(F):
            ij = i + F * j
            E = acc[off_e + ij * E_WORDS:off_e + (ij + 1) * E_WORDS]
            isl, jsl = slice(4 + 8 * i, 12 + 8 * i), slice(4 + 8 * j, 12 + 8 * j)
            Hs[isl, :4] += adH[ij] @ E[:32].reshape(8, 4)
            Hs[jsl, :4] += adT[ij] @ E[:32].reshape(8, 4)
            bs[isl] += adH[ij] @ E[32:]
            bs[jsl] += adT[ij] @ E[32:]
            for k in range(F):
                D = acc[off_d + (ij + k * F * F) * D_WORDS:off_d + (ij + k * F * F + 1) * D_WORDS]
                if D[64] == 0:
                    continue
                ik, ksl, M = i + F * k, slice(4 + 8 * k, 12 + 8 * k), D[:64].reshape(8, 8)
                Hs[isl, isl] += adH[ij] @ M @ adH[ik].T
                Hs[jsl, ksl] += adT[ij] @ M @ adT[ik].T
                Hs[jsl, isl] += adT[ij] @ M @ adH[ik].T
                Hs[isl, ksl] += adH[ij] @ M @ adT[ik].T
    C = acc[off_c:].reshape(F, C_WORDS).sum(axis=0)
    Hs[:4, :4], bs[:4] = C[:16].reshape(4, 4), C[16:]
    for h in range(F):
        hs = slice(4 + 8 * h, 12 + 8 * h)
        Hs[:4, hs] = Hs[hs, :4].T
    return HA, bA, Hs, bs


def stitch_bound(F, acc, acc_bound, adH, adT, issue=False):
    """issue=True: gamma_24 (|A| |M| |B|) plus the propagated accumulator bound, as the issue states it.  Otherwise the entrywise bound of a stitched matrix against another evaluation of the same formula: the standard product bound
    gamma_k (|A| |M| |B|) with k = 24 for the 8 x 8 triple product as the two-stage sums form it, plus one rounding per block addition
    into an entry (at most F^2 + 2 of them, the transposed add included), for BOTH evaluations; plus the accumulators' own bound
    propagated through |A| . |B|.  The count word of a block (1.0 per term) is kept, so the num == 0 skips are the same."""
    keep = np.abs(acc)
    k = 24 if issue else 24 + F * F + 2
    g = k * 2.0 ** -53 / (1 - k * 2.0 ** -53)
    prod = stitch(F, keep, np.abs(adH), np.abs(adT))
    b = acc_bound.copy()
    e, d, c, _ = acc_offsets(F)
    b[91:e:TOP_WORDS] = keep[91:e:TOP_WORDS]
    b[d + 64:c:D_WORDS] = keep[d + 64:c:D_WORDS]
    prop = stitch(F, b, np.abs(adH), np.abs(adT))
    return [(1 if issue else 2) * g * p + (1 + g) * q for p, q in zip(prod, prop)]
