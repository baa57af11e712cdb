"""A numpy restatement of dso::CoarseInitializer (reference src/init/CoarseInitializer.cpp) in the reference's own loop order: what
tests/test_init_oracle.py holds csrc/eds_init.hpp against.  Per tap and per point the arithmetic is fp32 in the C++ expressions' order
(vectorised over the points where the reference's loop has no dependence between its iterations, which changes no bit); optReg,
resetPoints and propagateUp are the serial loops, in index order, in place; E, acc9 and acc9SC are the reference's fp32 accumulators with
their three tiers (MatrixAccumulators.h), acc9 four taps to an SSE register.  The 8 x 8 solve is LAPACK's in fp32 (standing for Eigen's
pivoted fp32 ldlt), SE3::exp and log are closed forms over libm in fp64.  Two things follow csrc/eds_init.hpp instead of Eigen, because
the per-tap comparison is bit for bit "given the same pose": Ki is the closed form of the inverse of K in fp64, and the dot product of
doStep is summed left to right."""
import math

import numpy as np

import init_harness as ih

f32 = np.float32
PATTERN = ((0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2))
TRI = [(a, b) for a in range(9) for b in range(a, 9)]


def pyramid(img, levels):
    """per level h x w x 3 (colour, dx, dy): makeImages with the flat-index gradient rule"""
    out, c = [], np.asarray(img, dtype=f32)
    for l in range(levels):
        if l:
            c = f32(0.25) * (((c[0::2, 0::2] + c[0::2, 1::2]) + c[1::2, 0::2]) + c[1::2, 1::2])
        h, w = c.shape
        flat = c.ravel()
        dx, dy = np.zeros(h * w, f32), np.zeros(h * w, f32)
        idx = np.arange(w, w * (h - 1))
        with np.errstate(all="ignore"):
            gx = f32(0.5) * (flat[idx + 1] - flat[idx - 1])
            gy = f32(0.5) * (flat[idx + w] - flat[idx - w])
        dx[idx] = np.where(np.isfinite(gx), gx, f32(0))
        dy[idx] = np.where(np.isfinite(gy), gy, f32(0))
        out.append(np.stack([flat, dx, dy], axis=1).reshape(h, w, 3))
    return out


def interp(img, x, y):
    """getInterpolatedElement33 at float32 (x, y): n x 3"""
    h, w, _ = img.shape
    flat = img.reshape(-1, 3)
    ix, iy = x.astype(np.int32), y.astype(np.int32)
    dx, dy = x - ix.astype(f32), y - iy.astype(f32)
    dxdy = dx * dy
    bp = ix + iy * w
    return ((dxdy[:, None] * flat[bp + 1 + w] + (dy - dxdy)[:, None] * flat[bp + w]) + (dx - dxdy)[:, None] * flat[bp + 1]) + \
        (f32(1) - dx - dy + dxdy)[:, None] * flat[bp]


class Acc:
    """an fp32 accumulator of `k` entries x 4 SSE lanes with the reference's tiers"""

    def __init__(self, k):
        self.d, self.d1k, self.d1m = (np.zeros((k, 4), f32) for _ in range(3))
        self.n1 = self.n1k = 0
        self.num = 0

    def shift(self, force):
        if self.n1 > 1000 or force:
            self.d1k = self.d + self.d1k; self.n1k += self.n1; self.n1 = 0; self.d[:] = 0
        if self.n1k > 1000 or force:
            self.d1m = self.d1k + self.d1m; self.n1k = 0; self.d1k[:] = 0

    def update(self, v, lanes):
        self.d[:, :lanes] = self.d[:, :lanes] + v
        self.num += lanes; self.n1 += 1
        self.shift(False)

    def update_many(self, U, lanes):
        """U[m]: m updates in order (m x k x lanes); the running fp32 sums are numpy's sequential accumulate"""
        i = 0
        while i < len(U):
            take = min(len(U) - i, 1001 - self.n1)
            blk = np.concatenate([self.d[None, :, :lanes], U[i:i + take]], axis=0)
            self.d[:, :lanes] = np.add.accumulate(blk, axis=0, dtype=f32)[-1]
            self.n1 += take; self.num += take * lanes; i += take
            self.shift(False)

    def finish(self):
        self.shift(True)
        m = self.d1m
        return ((m[:, 0] + m[:, 1]) + m[:, 2]) + m[:, 3]


def se3_exp(xi):
    u, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = math.sqrt(float(w @ w))
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        R, V = np.eye(3) + W, np.eye(3) + 0.5 * W
    else:
        R = np.eye(3) + math.sin(th) / th * W + (1 - math.cos(th)) / th ** 2 * W @ W
        V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * W + (th - math.sin(th)) / th ** 3 * W @ W
    return R, V @ u


def se3_log_upsilon(R, t):
    c = min(1.0, max(-1.0, (np.trace(R) - 1) / 2))
    th = math.acos(c)
    if th < 1e-10:
        w = np.zeros(3)
    else:
        w = th / (2 * math.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    c2 = 1 / 12 if th < 1e-10 else (1 - th / (2 * math.tan(th / 2))) / th ** 2
    return (np.eye(3) - 0.5 * W + c2 * W @ W) @ t


class Oracle:
    def __init__(self, c):
        self.c, self.levels = c, c.levels
        self.prm = ih.default_params(**c.prm)[0]
        fx, fy, cx, cy = (f32(v) for v in c.K)
        self.K = [(fx, fy, cx, cy)]
        for l in range(1, c.levels):
            p = self.K[-1]
            self.K.append((f32(float(p[0]) * 0.5), f32(float(p[1]) * 0.5), f32((float(cx) + 0.5) / (1 << l) - 0.5), f32((float(cy) + 0.5) / (1 << l) - 0.5)))
        self.Kd = [(float(fx) / (1 << l), float(fy) / (1 << l), float(cx) if l == 0 else (float(cx) + 0.5) / (1 << l) - 0.5,
                    float(cy) if l == 0 else (float(cy) + 0.5) / (1 << l) - 0.5) for l in range(c.levels)]
        self.first = pyramid(c.first, c.levels)
        self.new = None
        self.pts, self.nb, self.parent = [], c.nb, c.parent
        for l in range(c.levels):                                  # setFirst :718-749
            st = c.status[l]
            h, w = st.shape
            p = np.zeros(len(c.uv[l]), ih.POINT)
            k = 0
            for y in range(3, h - 4):
                for x in range(3, w - 4):
                    if st[y, x] != 0:
                        p[k]["u"], p[k]["v"] = f32(x + 0.1), f32(y + 0.1)
                        p[k]["idepth"] = p[k]["iR"] = p[k]["idepth_new"] = 1
                        p[k]["isGood"] = 1
                        p[k]["my_type"] = st[y, x]
                        p[k]["outlierTH"] = f32(8) * self.prm["outlier_th"]
                        k += 1
            assert k == len(p)
            self.pts.append(p)
        self.jb = [np.zeros((len(p), 10), f32) for p in self.pts]
        self.jb_new = [np.zeros((len(p), 10), f32) for p in self.pts]
        self.R, self.t, self.aff = np.eye(3), np.zeros(3), np.zeros(2)
        if c.pose_guess is not None:
            self.R, self.t = c.pose_guess[:, :3].copy(), c.pose_guess[:, 3].copy()
        self.snapped, self.frame_id, self.snapped_at = False, 0, 0

    def set_new(self, img):
        self.new = pyramid(img, self.levels)

    # ---- calcResAndGS :265-522 ---------------------------------------------------------------------------------------------------------
    def first_loop(self, lvl, R, t, a, b):
        """the loop :292-428 without its sums: per tap residual and hw, the rows, and the points' new state"""
        P, s = self.pts[lvl], self.prm
        n = len(P)
        fxl, fyl, cxl, cyl = self.K[lvl]
        fxd, fyd, cxd, cyd = self.Kd[lvl]
        Ki = np.array([[1.0 / fxd, 0, -cxd / fxd], [0, 1.0 / fyd, -cyd / fyd], [0, 0, 1.0]])
        RKi = np.empty((3, 3), f32)
        for i in range(3):
            RKi[i, 0] = f32(R[i, 0] * Ki[0, 0]); RKi[i, 1] = f32(R[i, 1] * Ki[1, 1])
            RKi[i, 2] = f32((R[i, 0] * Ki[0, 2] + R[i, 1] * Ki[1, 2]) + R[i, 2])
        tf = np.asarray(t, dtype=np.float64).astype(f32)
        ra, rb = f32(math.exp(a)), f32(b)
        h, w, _ = self.new[lvl].shape
        huber = s["huber_th"]
        alive = P["isGood"].astype(bool).copy()
        energy, maxstep = np.zeros(n, f32), np.full(n, f32(1e10))
        J = np.zeros((n, 8, 9), f32)
        row = np.zeros((n, 10), f32)
        taps = np.full((n, 8, 2), np.nan, f32)
        idn = P["idepth_new"]
        with np.errstate(all="ignore"):
            for k, (dx, dy) in enumerate(PATTERN):
                x, y = P["u"] + f32(dx), P["v"] + f32(dy)
                pt = [((RKi[i, 0] * x + RKi[i, 1] * y) + RKi[i, 2] * f32(1)) + tf[i] * idn for i in range(3)]
                u, v = pt[0] / pt[2], pt[1] / pt[2]
                Ku, Kv = fxl * u + cxl, fyl * v + cyl
                nid = idn / pt[2]
                ok = alive & (Ku > 1) & (Kv > 1) & (Ku < f32(w - 2)) & (Kv < f32(h - 2)) & (nid > 0)
                alive &= ok
                m = np.nonzero(ok)[0]
                hit = interp(self.new[lvl], Ku[m], Kv[m])
                rl = interp(self.first[lvl], x[m], y[m])[:, 0]
                fin = np.isfinite(rl) & np.isfinite(hit[:, 0])
                alive[m[~fin]] = False
                m, hit, rl = m[fin], hit[fin], rl[fin]
                u, v, nid, p2 = u[m], v[m], nid[m], pt[2][m]
                res = hit[:, 0] - ra * rl - rb
                hw = np.where(np.abs(res) < huber, f32(1), huber / np.abs(res)).astype(f32)
                taps[m, k, 0], taps[m, k, 1] = res, hw
                energy[m] = energy[m] + hw * res * res * (f32(2) - hw)
                dxdd, dydd = (tf[0] - tf[2] * u) / p2, (tf[1] - tf[2] * v) / p2
                hw = np.where(hw < 1, np.sqrt(hw), hw).astype(f32)
                dxI, dyI = hw * hit[:, 1] * fxl, hw * hit[:, 2] * fyl
                Jk = np.stack([nid * dxI, nid * dyI, -nid * (u * dxI + v * dyI), -u * v * dxI - (f32(1) + v * v) * dyI,
                               (f32(1) + u * u) * dxI + u * v * dyI, -v * dxI + u * dyI, -hw * ra * rl, -hw * f32(1), hw * res], axis=1)
                J[m, k] = Jk
                dd = dxI * dxdd + dyI * dydd
                sx, sy = dxdd * fxl, dydd * fyl
                ms = f32(1) / np.sqrt(sx * sx + sy * sy)
                maxstep[m] = np.where(ms < maxstep[m], ms, maxstep[m])
                row[m, :9] = row[m, :9] + Jk * dd[:, None]
                row[m, 9] = row[m, 9] + dd * dd
        was_good = P["isGood"].astype(bool)
        good_new = alive & ~(energy > P["outlierTH"] * f32(20))
        return dict(J=J, row=row, taps=taps, energy=energy, maxstep=maxstep, good_new=good_new, was_good=was_good)

    def calc(self, lvl, R, t, a, b):
        P, s = self.pts[lvl], self.prm
        n = len(P)
        fl = self.first_loop(lvl, R, t, a, b)
        J, good_new, was_good = fl["J"], fl["good_new"], fl["was_good"]
        P["maxstep"] = fl["maxstep"]
        self.jb_new[lvl][was_good] = fl["row"][was_good]
        E, acc9 = Acc(1), Acc(45)
        e_terms = np.where(good_new, fl["energy"], P["energy"][:, 0]).astype(f32)
        E.update_many(e_terms[:, None, None], 1)                  # the accumulators, in the loop's order
        Jg = J[good_new].reshape(-1, 2, 4, 9)                     # per good point: two SSE updates of four taps
        prod = np.stack([Jg[..., a_] * Jg[..., b_] for a_, b_ in TRI], axis=2).reshape(-1, 45, 4)
        acc9.update_many(prod, 4)
        terms = {"E": e_terms.astype(np.float64), "acc9": prod.astype(np.float64).sum(axis=(0, 2)), "acc9_abs": np.abs(prod.astype(np.float64)).sum(axis=(0, 2)),
                 "n_good": int(good_new.sum())}
        P["energy_new"][~good_new] = P["energy"][~good_new]
        P["energy_new"][good_new, 0] = fl["energy"][good_new]
        P["isGood_new"] = good_new
        EA = E.finish()[0]
        H9 = acc9.finish()
        idn = P["idepth_new"]
        P["energy_new"][good_new, 1] = ((idn - f32(1)) * (idn - f32(1)))[good_new]        # :450; E is already finished: EAlpha.A stays 0
        tsq = float((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        alphaEnergy = f32(float(s["alpha_w"]) * (0.0 + tsq * n))
        if alphaEnergy > s["alpha_k"] * f32(n):
            alphaOpt, alphaEnergy = f32(0), s["alpha_k"] * f32(n)
        else:
            alphaOpt = s["alpha_w"]
        sc = Acc(45)
        jb = self.jb_new[lvl]
        cw = s["coupling_weight"]
        g = np.nonzero(good_new)[0]                               # :474-496, every row on its own
        r = jb[g]
        P["lastHessian_new"][g] = r[:, 9]
        r[:, 8] = r[:, 8] + alphaOpt * (idn[g] - f32(1)); r[:, 9] = r[:, 9] + alphaOpt
        if alphaOpt == 0:
            r[:, 8] = r[:, 8] + cw * (idn[g] - P["iR"][g]); r[:, 9] = r[:, 9] + cw
        r[:, 9] = f32(1) / (f32(1) + r[:, 9])
        jb[g] = r
        wgt, cols = r[:, 9], []
        for a_ in range(9):
            cols.append(r[:, a_] * r[:, a_] * wgt)
            jw = r[:, a_] * wgt
            cols += [r[:, b_] * jw for b_ in range(a_ + 1, 9)]
        v = np.stack(cols, axis=1).astype(f32)
        sc.update_many(v[:, :, None], 1)
        terms["sc"], terms["sc_abs"] = v.astype(np.float64).sum(axis=0), np.abs(v.astype(np.float64)).sum(axis=0)
        S9 = sc.finish()

        def mat(S):
            M = np.zeros((9, 9), f32)
            for q, (a_, b_) in enumerate(TRI):
                M[a_, b_] = M[b_, a_] = S[q]
            return M
        M, Msc = mat(H9), mat(S9)
        H, bb, Hsc, bsc = M[:8, :8].copy(), M[:8, 8].copy(), Msc[:8, :8].copy(), Msc[:8, 8].copy()
        tlog = se3_log_upsilon(R, np.asarray(t, dtype=np.float64)).astype(f32)
        for i in range(3):
            H[i, i] = H[i, i] + alphaOpt * f32(n)
            bb[i] = bb[i] + tlog[i] * alphaOpt * f32(n)
        self.terms = terms
        return H, bb, Hsc, bsc, np.array([EA, alphaEnergy, f32(2 * n)], f32)

    def calc_ec(self, lvl):                                        # :531-551
        P = self.pts[lvl]
        if not self.snapped:
            return np.array([0, 0, len(P)], f32)
        A = Acc(2)
        g = np.nonzero(P["isGood_new"])[0]
        rO, rN = P["idepth"][g] - P["iR"][g], P["idepth_new"][g] - P["iR"][g]
        terms = np.stack([rO * rO, rN * rN], axis=1).astype(f32)
        self.ec_terms = terms.astype(np.float64)
        A.update_many(terms[:, :, None], 1)
        A.shift(True)
        cw = self.prm["coupling_weight"]
        return np.array([cw * A.d1m[0, 0], cw * A.d1m[1, 0], f32(int(P["isGood_new"].sum()))], f32)

    # ---- the loops that depend on their own order -----------------------------------------------------------------------------------------
    def opt_reg(self, lvl, jacobi=False):                          # :552-587
        P, nb = self.pts[lvl], self.nb[lvl]
        if not self.snapped:
            P["iR"] = 1
            return
        rw = self.prm["reg_weight"]
        src = P["iR"].copy() if jacobi else P["iR"]
        for i in range(len(P)):
            if not P["isGood"][i]:
                continue
            idnn = [src[j] for j in nb[i] if j != -1 and P["isGood"][j]]
            if len(idnn) > 2:
                P["iR"][i] = (f32(1) - rw) * P["idepth"][i] + rw * sorted(idnn)[len(idnn) // 2]

    def reset_points(self, lvl, jacobi=False):                     # :775-802
        P, nb = self.pts[lvl], self.nb[lvl]
        P["energy"] = 0
        P["idepth_new"] = P["idepth"]
        if lvl != self.levels - 1:
            return
        good, iR = (P["isGood"].copy(), P["iR"].copy()) if jacobi else (P["isGood"], P["iR"])
        for i in range(len(P)):
            if P["isGood"][i]:
                continue
            snd, sn = f32(0), f32(0)
            for j in nb[i]:
                if j == -1 or not good[j]:
                    continue
                snd = snd + iR[j]; sn = sn + f32(1)
            if sn > 0:
                P["isGood"][i] = 1
                P["iR"][i] = P["idepth"][i] = P["idepth_new"][i] = snd / sn

    def propagate_up(self, src):                                   # :591-630
        S, T = self.pts[src], self.pts[src + 1]
        T["iR"] = 0
        num = np.zeros(len(T), f32)
        for i in range(len(S)):
            if not S["isGood"][i]:
                continue
            p = self.parent[src][i]
            T["iR"][p] = T["iR"][p] + S["iR"][i] * S["lastHessian"][i]
            num[p] = num[p] + S["lastHessian"][i]
        m = num > 0
        T["iR"][m] = T["iR"][m] / num[m]
        T["idepth"][m] = T["iR"][m]
        T["isGood"][m] = 1
        self.opt_reg(src + 1)

    def propagate_down(self, src):                                 # :632-660
        S, T = self.pts[src], self.pts[src - 1]
        par = S[self.parent[src - 1]]
        use = par["isGood"].astype(bool) & ~(par["lastHessian"].astype(np.float64) < 0.1)
        bad = use & ~T["isGood"].astype(bool)
        good = use & T["isGood"].astype(bool)
        with np.errstate(all="ignore"):
            newiR = (T["iR"] * T["lastHessian"] * f32(2) + par["iR"] * par["lastHessian"]) / (T["lastHessian"] * f32(2) + par["lastHessian"])
        for f in ("iR", "idepth", "idepth_new"):
            T[f][bad] = par["iR"][bad]
            T[f][good] = newiR[good]
        T["isGood"][bad] = 1
        T["lastHessian"][bad] = 0
        self.opt_reg(src - 1)

    # ---- doStep :804-832, applyStep :834-851 ---------------------------------------------------------------------------------------------
    def do_step(self, lvl, lam, inc):
        P, jb = self.pts[lvl], self.jb[lvl]
        lam, inc = f32(lam), np.asarray(inc, dtype=f32)
        dot = jb[:, 0] * inc[0]
        for q in range(1, 8):
            dot = dot + jb[:, q] * inc[q]
        b = jb[:, 8] + dot
        with np.errstate(all="ignore"):
            step = -b * jb[:, 9] / (f32(1) + lam)
            ms = f32(0.25) * P["maxstep"]
            ms = np.where(ms > f32(1e10), f32(1e10), ms)
            step = np.where(step > ms, ms, step)
            step = np.where(step < -ms, -ms, step)
            nid = P["idepth"] + step
            nid = np.where(nid.astype(np.float64) < 1e-3, f32(1e-3), nid)
            nid = np.where(nid > 50, f32(50), nid).astype(f32)
        g = P["isGood"].astype(bool)
        P["idepth_new"][g] = nid[g]

    def apply_step(self, lvl):
        P = self.pts[lvl]
        g = P["isGood"].astype(bool)
        P["idepth"][~g] = P["iR"][~g]; P["idepth_new"][~g] = P["iR"][~g]
        P["energy"][g] = P["energy_new"][g]
        P["idepth"][g] = P["idepth_new"][g]
        P["lastHessian"][g] = P["lastHessian_new"][g]
        P["isGood"][g] = P["isGood_new"][g]
        self.jb[lvl], self.jb_new[lvl] = self.jb_new[lvl], self.jb[lvl]

    # ---- trackFrame :75-262 --------------------------------------------------------------------------------------------------------------
    def track_frame(self, img, exposure, exposure_first, snapped_threshold):
        s = self.prm
        self.set_new(img)
        wM = np.array([s["scale_xi_rot"]] * 3 + [s["scale_xi_trans"]] * 3 + [s["scale_a"], s["scale_b"]], f32)
        if not self.snapped:
            self.t = np.zeros(3)
            for P in self.pts:
                P["iR"] = 1; P["idepth_new"] = 1; P["lastHessian"] = 0
        R, t, a, b = self.R.copy(), self.t.copy(), self.aff[0], self.aff[1]
        if exposure_first > 0 and exposure > 0:
            a, b = float(f32(math.log(f32(exposure) / f32(exposure_first)))), 0.0
        decisions = []
        for lvl in range(self.levels - 1, -1, -1):
            if lvl < self.levels - 1:
                self.propagate_down(lvl + 1)
            self.reset_points(lvl)
            H, bb, Hsc, bsc, res_old = self.calc(lvl, R, t, a, b)
            self.apply_step(lvl)
            lam, fails, iteration = f32(0.1), 0, 0
            hh, ww, _ = self.new[lvl].shape
            n = len(self.pts[lvl])
            while True:
                Hl = H.copy()
                for i in range(8):
                    Hl[i, i] = Hl[i, i] * (f32(1) + lam)
                k = f32(1) / (f32(1) + lam)
                Hl = Hl - Hsc * k
                bl = bb - bsc * k
                scl = f32(0.01) / f32(ww * hh)
                Hl = (wM[:, None] * Hl * wM[None, :] * scl).astype(f32)
                bl = (wM * bl * scl).astype(f32)
                inc = np.zeros(8, f32)
                with np.errstate(all="ignore"):
                    try:
                        if s["fix_affine"]:
                            inc[:6] = -(wM[:6] * np.linalg.solve(Hl[:6, :6], bl[:6]).astype(f32))
                        else:
                            inc = -(wM * np.linalg.solve(Hl, bl).astype(f32))
                    except np.linalg.LinAlgError:
                        inc[:] = np.nan
                Ri, ti = se3_exp(inc[:6].astype(np.float64))
                Rn, tn = Ri @ R, Ri @ t + ti
                an, bn = a + float(inc[6]), b + float(inc[7])
                self.do_step(lvl, lam, inc)
                Hn, bbn, Hscn, bscn, res_new = self.calc(lvl, Rn, tn, an, bn)
                reg = self.calc_ec(lvl)
                eNew = res_new[0] + res_new[1] + reg[1]
                eOld = res_old[0] + res_old[1] + reg[0]
                accept = bool(eOld > eNew)
                decisions.append((1 if accept else 0) | (lvl << 1))
                if accept:
                    if res_new[1] == s["alpha_k"] * f32(n):
                        self.snapped = True
                    H, bb, Hsc, bsc, res_old = Hn, bbn, Hscn, bscn, res_new
                    R, t, a, b = Rn, tn, an, bn
                    self.apply_step(lvl)
                    self.opt_reg(lvl)
                    lam = f32(float(lam) * 0.5)
                    fails = 0
                    if float(lam) < 0.0001:
                        lam = f32(0.0001)
                else:
                    fails += 1
                    lam = lam * f32(4)
                    if lam > 10000:
                        lam = f32(10000)
                nrm = f32(np.sqrt(np.sum(inc.astype(f32) ** 2, dtype=f32)))
                if not (nrm > f32(1e-4)) or iteration >= s["max_iterations"][lvl] or fails >= 2:
                    break
                iteration += 1
        self.R, self.t, self.aff = R, t, np.array([a, b])
        for i in range(self.levels - 1):
            self.propagate_up(i)
        self.frame_id += 1
        if not self.snapped:
            self.snapped_at = 0
        if self.snapped and self.snapped_at == 0:
            self.snapped_at = self.frame_id
        return dict(T=np.concatenate([R, t[:, None]], axis=1), aff=np.array([a, b]), snapped=int(self.snapped), frame_id=self.frame_id,
                    snapped_at=self.snapped_at, ready=int(self.snapped and self.frame_id > self.snapped_at + snapped_threshold),
                    decisions=decisions, latest_res=res_old)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
