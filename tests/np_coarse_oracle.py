"""A numpy oracle of dso::CoarseTracker written from the reference text (src/tracking/CoarseTracker.cpp:93-701,
src/tracking/HessianBlocks.cpp:139-202), independent of csrc/eds_coarse.hpp: float32 per point in the reference's operand order, the sums
of the fp32 terms taken EXACTLY (math.fsum), the solves by numpy.linalg.solve in fp64, libm sin / cos / exp.  For every accept test it
records the relative margin |new - old| / old.  The keyword switches (list_order, collision_order, padded, fy_is_fx) exist only for
tests/test_coarse_oracle.py, which shows that the cases tell these variants apart."""
import math

import numpy as np

f32 = np.float32
SCALE = np.array([1, 1, 1, 1, 1, 1, 10, 1000], dtype=np.float64)           # SCALE_XI_ROT, _TRANS, _A, _B (HessianBlocks.h:58-65)
DEFAULTS = dict(huber_th=9.0, coarse_cutoff_th=20.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8)      # settings.cpp:119-138


def params(**over):
    p = {k: float(f32(v)) for k, v in DEFAULTS.items()}
    p.update({k: float(f32(v)) for k, v in over.items()})
    return p


def make_k(W, H, levels, fx, fy, cx, cy, fy_is_fx=False):
    """:93-122; Ki in closed form, fp32"""
    K = [dict(w=W, h=H, fx=f32(fx), fy=f32(fx if fy_is_fx else fy), cx=f32(cx), cy=f32(cy))]
    for l in range(1, levels):
        p = K[l - 1]
        K.append(dict(w=W >> l, h=H >> l, fx=f32(np.float64(p["fx"]) * 0.5), fy=f32(np.float64(p["fy"]) * 0.5),
                      cx=f32((np.float64(K[0]["cx"]) + 0.5) / (1 << l) - 0.5), cy=f32((np.float64(K[0]["cy"]) + 0.5) / (1 << l) - 0.5)))
    for k in K:
        k["fxi"], k["fyi"] = f32(1) / k["fx"], f32(1) / k["fy"]
        k["cxi"], k["cyi"] = -k["cx"] / k["fx"], -k["cy"] / k["fy"]
    return K


def make_images(color, levels):
    """HessianBlocks.cpp:139-202: per level an h x w x 3 array (colour, dx, dy)"""
    out, c = [], np.ascontiguousarray(color, dtype=f32)
    for l in range(levels):
        if l > 0:
            p = out[l - 1][:, :, 0]
            c = f32(0.25) * (((p[0::2, 0::2] + p[0::2, 1::2]) + p[1::2, 0::2]) + p[1::2, 1::2])
        h, w = c.shape
        flat = c.ravel()
        dx, dy = np.zeros(h * w, f32), np.zeros(h * w, f32)
        i = np.arange(w, w * (h - 1))
        with np.errstate(all="ignore"):
            gx = f32(0.5) * (flat[i + 1] - flat[i - 1])
            gy = f32(0.5) * (flat[i + w] - flat[i - w])
        dx[i], dy[i] = np.where(np.isfinite(gx), gx, f32(0)), np.where(np.isfinite(gy), gy, f32(0))
        out.append(np.stack([c, dx.reshape(h, w), dy.reshape(h, w)], axis=2).astype(f32))
    return out


def make_depth(K, ref_images, cp, hdif, list_order="row", collision_order="input"):
    """:126-283; returns idepth[l], weightSums[l] (h x w), pc[l] (n x 4: u, v, idepth, colour), dropped"""
    levels, W, H = len(K), K[0]["w"], K[0]["h"]
    cp, hdif = np.asarray(cp, dtype=f32).reshape(-1, 3), np.asarray(hdif, dtype=f32)
    idp, ws = [np.zeros(k["w"] * k["h"], f32) for k in K], [np.zeros(k["w"] * k["h"], f32) for k in K]
    dropped = 0
    order = range(len(cp)) if collision_order == "input" else range(len(cp) - 1, -1, -1)
    with np.errstate(all="ignore"):
        for i in order:
            xf, yf = cp[i, 0] + f32(0.5), cp[i, 1] + f32(0.5)
            if not (xf > -1 and xf < W and yf > -1 and yf < H):
                dropped += 1
                continue
            pix = int(xf) + W * int(yf)
            weight = np.sqrt(f32(1e-3 / (np.float64(hdif[i]) + 1e-12)))
            idp[0][pix] += cp[i, 2] * weight
            ws[0][pix] += weight
        for l in range(1, levels):
            for dst, src in ((idp, idp), (ws, ws)):
                p = src[l - 1].reshape(K[l - 1]["h"], K[l - 1]["w"])
                dst[l] = (((p[0::2, 0::2] + p[0::2, 1::2]) + p[1::2, 0::2]) + p[1::2, 1::2]).ravel().astype(f32)
        pcs = []
        for l in range(levels):
            w, h = K[l]["w"], K[l]["h"]
            bak, dep = ws[l].copy(), idp[l].copy()
            i = np.arange(w, w * h - w)
            i = i[bak[i] <= 0]
            offs = (1 + w, -1 - w, w - 1, -w + 1) if l < 2 else (1, -1, w, -w)
            s, num, numn = np.zeros(len(i), f32), np.zeros(len(i), f32), np.zeros(len(i), f32)
            for o in offs:
                j = i + o
                ok = (j >= 0) & (j < w * h)
                jj = np.where(ok, j, 0)
                ok &= bak[jj] > 0
                s, num, numn = np.where(ok, s + dep[jj], s), np.where(ok, num + bak[jj], num), np.where(ok, numn + f32(1), numn)
            hit = numn > 0
            idp[l][i[hit]], ws[l][i[hit]] = s[hit] / numn[hit], num[hit] / numn[hit]
            # normalisation over the interior; the `continue` branch leaves weightSums as it is
            ID, WS, col = idp[l].reshape(h, w), ws[l].reshape(h, w), ref_images[l][:, :, 0]
            inner = np.zeros((h, w), bool)
            inner[2:h - 2, 2:w - 2] = True
            pos = inner & (WS > 0)
            ID[pos] = ID[pos] / WS[pos]
            good = pos & np.isfinite(col) & (ID > 0)
            ID[inner & ~good] = f32(-1)
            WS[inner & (good | ~pos)] = f32(1)
            v, u = np.nonzero(good) if list_order == "row" else np.nonzero(good.T)[::-1]
            pcs.append(np.stack([u.astype(f32), v.astype(f32), ID[v, u], col[v, u]], axis=1).astype(f32).reshape(-1, 4))
    return [a.reshape(K[l]["h"], K[l]["w"]) for l, a in enumerate(idp)], [a.reshape(K[l]["h"], K[l]["w"]) for l, a in enumerate(ws)], pcs, dropped


def from_to_exposure(exp_f, exp_t, g2f, g2t):
    """NumType.h:175-187"""
    ef, et = f32(exp_f), f32(exp_t)
    if ef == 0 or et == 0:
        ef = et = f32(1)
    a = math.exp(g2t[0] - g2f[0]) * float(et) / float(ef)
    return a, g2t[1] - a * g2f[1]


class Oracle:
    def __init__(self, H, W, levels, K, prm=None, **variant):
        self.v = variant
        self.K = make_k(W, H, levels, *K, fy_is_fx=variant.get("fy_is_fx", False))
        self.levels, self.prm = levels, params(**(prm or {}))

    def set_ref(self, image, cp, hdif, exposure=1.0, aff=(0.0, 0.0)):
        self.ref = make_images(image, self.levels)
        self.idepth, self.wsum, self.pc, self.dropped = make_depth(self.K, self.ref, cp, hdif, self.v.get("list_order", "row"),
                                                                   self.v.get("collision_order", "input"))
        self.exp_ref, self.aff_ref = exposure, (float(aff[0]), float(aff[1]))

    def set_new(self, image, exposure=1.0):
        self.new = make_images(image, self.levels)
        self.exp_new = exposure

    def calc_res(self, lvl, T, aff, cutoff):
        """:349-498 — the rows (one per list entry) and rs with E and the flow sums exact"""
        k, pc = self.K[lvl], self.pc[lvl]
        T = np.asarray(T, dtype=np.float64).reshape(3, 4)
        R, t = T[:, :3].astype(f32), T[:, 3].astype(f32)
        Ki = np.array([[k["fxi"], 0, k["cxi"]], [0, k["fyi"], k["cyi"]], [0, 0, 1]], dtype=f32)
        with np.errstate(all="ignore"):
            RKi = np.array([[(R[i, 0] * Ki[0, j] + R[i, 1] * Ki[1, j]) + R[i, 2] * Ki[2, j] for j in range(3)] for i in range(3)], dtype=f32)
            a64, b64 = from_to_exposure(self.exp_ref, self.exp_new, self.aff_ref, aff)
            aff0, aff1 = f32(a64), f32(b64)
            hub, cut = f32(self.prm["huber_th"]), f32(cutoff)
            max_energy = f32(2) * hub * cut - hub * hub
            x, y, idp, col = pc[:, 0], pc[:, 1], pc[:, 2], pc[:, 3]
            one = f32(1)

            def proj(M, sign):
                p = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * one) + sign * (t[i] * idp) for i in range(3)]
                u, v = p[0] / p[2], p[1] / p[2]
                return u, v, k["fx"] * u + k["cx"], k["fy"] * v + k["cy"], p[2]
            u, v, Ku, Kv, z = proj(RKi, one)
            new_idepth = idp / z
            n = len(pc)
            flow = np.zeros(n, bool)
            if lvl == 0:
                flow[0::32] = True
            sh = lambda a, b: (a - x) * (a - x) + (b - y) * (b - y)
            _, _, KuT, KvT, _ = proj(Ki, one)
            _, _, KuT2, KvT2, _ = proj(Ki, -one)
            _, _, Ku3, Kv3, _ = proj(RKi, -one)
            t1, t2, rt1, rt2 = sh(KuT, KvT), sh(KuT2, KvT2), sh(Ku, Kv), sh(Ku3, Kv3)
            inb = (Ku > 2) & (Kv > 2) & (Ku < k["w"] - 3) & (Kv < k["h"] - 3) & (new_idepth > 0)
            ix, iy = np.where(inb, Ku, 2).astype(np.int64), np.where(inb, Kv, 2).astype(np.int64)
            dx, dy = Ku - ix.astype(f32), Kv - iy.astype(f32)
            dxdy = dx * dy
            img = self.new[lvl]
            w11, w01, w10, w00 = dxdy, dy - dxdy, dx - dxdy, one - dx - dy + dxdy
            hit = (w11[:, None] * img[iy + 1, ix + 1] + w01[:, None] * img[iy + 1, ix] + w10[:, None] * img[iy, ix + 1] + w00[:, None] * img[iy, ix])
            in_e = inb & np.isfinite(hit[:, 0])
            residual = hit[:, 0] - (aff0 * col + aff1)
            ar = np.abs(residual)
            hw = np.where(ar < hub, one, hub / ar).astype(f32)
            sat = in_e & (ar > cut)
            warped = in_e & ~sat
            e = np.where(sat, max_energy, hw * residual * residual * (f32(2) - hw)).astype(f32)
        rows = dict(in_e=in_e, warped=warped, flow=flow, energy=np.where(in_e, e, 0).astype(f32), idepth=new_idepth, u=u, v=v, dx=hit[:, 1], dy=hit[:, 2],
                    residual=residual, weight=hw, ref_color=col, shift_t_pos=t1, shift_t_neg=t2, shift_rt_pos=rt1, shift_rt_neg=rt2)
        nE, nflow = int(in_e.sum()), int(flow.sum())
        E = math.fsum(e[in_e].astype(np.float64))
        sT = math.fsum(np.concatenate([t1[flow], t2[flow]]).astype(np.float64)) if nflow else 0.0
        sRT = math.fsum(np.concatenate([rt1[flow], rt2[flow]]).astype(np.float64)) if nflow else 0.0
        with np.errstate(all="ignore"):
            rs = np.array([E, nE, sT / (2.0 * nflow + 0.1), 0.0, sRT / (2.0 * nflow + 0.1), float(f32(int(sat.sum())) / f32(nE))])
        # per sum: the number of terms and the sum of their magnitudes (the flow terms are squares, so that is the sum itself)
        abs_sums = dict(E=float(np.abs(e[in_e].astype(np.float64)).sum()), n=nE, n_flow=2 * nflow, sT=sT, sRT=sRT, den=2.0 * nflow + 0.1)
        return dict(rows=rows, rs=rs, abs=abs_sums, a=f32(a64), b0=f32(self.aff_ref[1]), k=k)

    def calc_gs(self, res):
        """:287-344 from calc_res's rows; returns H, b and per sum the bound n 2^-53 sum|term| scaled as H and b are"""
        r, k, m = res["rows"], res["k"], res["rows"]["warped"]
        g = lambda f: r[f][m].astype(f32)
        one = f32(1)
        with np.errstate(all="ignore"):
            dx, dy, u, v, idp = g("dx") * k["fx"], g("dy") * k["fy"], g("u"), g("v"), g("idepth")
            J = [idp * dx, idp * dy, f32(0) - idp * (u * dx + v * dy), f32(0) - ((u * v) * dx + dy * (one + v * v)),
                 (u * v) * dy + dx * (one + u * u), u * dy - v * dx, res["a"] * (res["b0"] - g("ref_color")), np.full(len(dx), -1, f32), g("residual")]
            wgt = g("weight")
            n = int(m.sum())
            npad = (n + 3) & ~3 if self.v.get("padded", True) else n
            inv = np.float64(f32(1) / f32(npad))
            S, A = np.zeros((9, 9)), np.zeros((9, 9))
            for a in range(9):
                for b in range(a, 9):
                    term = ((J[a] * wgt) * J[b]).astype(np.float64)
                    S[a, b] = S[b, a] = math.fsum(term)
                    A[a, b] = A[b, a] = np.abs(term).sum()
            sc = np.concatenate([SCALE, [1.0]])
            Hs, As = (S * inv) * sc[None, :] * sc[:, None], (A * inv) * sc[None, :] * sc[:, None] * n * 2.0 ** -53
        return Hs[:8, :8], Hs[:8, 8], As[:8, :8], As[:8, 8]

    def system(self, lvl, T, aff, cutoff):
        res = self.calc_res(lvl, T, aff, cutoff)
        return (res,) + self.calc_gs(res)

    def track(self, T_init, aff_init=(0.0, 0.0), coarsest=None, min_res=None):
        """:520-701"""
        p = self.prm
        ma, mb, cut0 = p["affine_opt_mode_a"], p["affine_opt_mode_b"], f32(p["coarse_cutoff_th"])
        coarsest = self.levels - 1 if coarsest is None else coarsest
        min_res = np.full(5, np.nan) if min_res is None else np.asarray(min_res, dtype=np.float64)
        T0 = np.asarray(T_init, dtype=np.float64).reshape(3, 4)
        T, aff = T0.copy(), [float(aff_init[0]), float(aff_init[1])]
        out = dict(T=T0.copy(), aff=np.array(aff), ok=False, last_residuals=np.full(5, np.nan), flow=np.full(3, 1000.0), iterations=np.zeros(5, int),
                   accepts=np.zeros(5, int), decisions=[], margins=[], branches=set(), flow_bound=np.zeros(3))
        limit, have_repeated, lvl = f32(0.001), False, coarsest
        with np.errstate(all="ignore"):
            while lvl >= 0:
                rep = f32(1)
                old = self.calc_res(lvl, T, aff, cut0 * rep)
                while old["rs"][5] > 0.6 and rep < 50:
                    rep = rep * f32(2)
                    old = self.calc_res(lvl, T, aff, cut0 * rep)
                    out["branches"].add("cutoff_doubled")
                H, b, _, _ = self.calc_gs(old)
                if old["rs"][1] == 0:
                    out["branches"].add("no_terms")
                lam = f32(0.01)
                for it in range((10, 20, 100, 100, 100)[lvl]):
                    Hl = H.copy()
                    Hl[np.arange(8), np.arange(8)] *= np.float64(f32(1) + lam)
                    inc = np.zeros(8)
                    try:
                        if ma < 0 and mb < 0:
                            inc[:6] = np.linalg.solve(Hl[:6, :6], -b[:6])
                        elif mb < 0:
                            inc[:7] = np.linalg.solve(Hl[:7, :7], -b[:7])
                        elif ma < 0:
                            sel = [0, 1, 2, 3, 4, 5, 7]
                            x = np.linalg.solve(Hl[np.ix_(sel, sel)], -b[sel])
                            inc[:6], inc[7] = x[:6], x[6]
                        else:
                            inc = np.linalg.solve(Hl, -b)
                    except np.linalg.LinAlgError:
                        inc = np.full(8, np.nan)
                    extrap = f32(1)
                    if lam < limit:
                        extrap = np.sqrt(np.sqrt(limit / lam))
                    inc = inc * np.float64(extrap)
                    incs = inc * SCALE
                    if not np.isfinite(incs.sum()):
                        incs = np.zeros(8)
                        out["branches"].add("step_zeroed")
                    Tn = se3_exp(incs[:6]) @ np.vstack([T, [0, 0, 0, 1]])
                    affn = [aff[0] + incs[6], aff[1] + incs[7]]
                    new = self.calc_res(lvl, Tn[:3], affn, cut0 * rep)
                    eo, en = old["rs"][0] / old["rs"][1], new["rs"][0] / new["rs"][1]
                    accept = bool(en < eo)
                    if np.isfinite(eo) and np.isfinite(en) and eo > 0:
                        out["margins"].append(abs(en - eo) / eo)
                    out["decisions"].append((lvl << 1) | int(accept))
                    out["iterations"][lvl] += 1
                    if accept:
                        H, b, _, _ = self.calc_gs(new)
                        old, T, aff = new, Tn[:3].copy(), affn
                        lam = lam * f32(0.5)
                        out["accepts"][lvl] += 1
                    else:
                        lam = lam * f32(4)
                        if lam < limit:
                            lam = limit
                    if not (np.linalg.norm(inc) > 1e-3):
                        out["branches"].add("small_inc")
                        break
                else:
                    out["branches"].add("max_iterations")
                last = np.sqrt(f32(old["rs"][0] / old["rs"][1]))
                out["last_residuals"][lvl], out["flow"] = float(last), old["rs"][2:5].copy()
                out["flow_bound"] = flow_bound(old)
                out["cutoff_repeat"] = float(rep)
                if float(last) > 1.5 * min_res[lvl]:
                    out["branches"].add("abort")
                    return out
                if rep > 1 and not have_repeated:
                    have_repeated = True
                    out["branches"].add("level_repeated")
                    continue
                lvl -= 1
        out["T"], out["aff"] = T, np.array(aff)
        if (ma != 0 and float(abs(f32(aff[0]))) > 1.2) or (mb != 0 and abs(f32(aff[1])) > 200):
            out["branches"].add("affine_out_of_range")
            return out
        ra, rb = from_to_exposure(self.exp_ref, self.exp_new, self.aff_ref, aff)
        with np.errstate(all="ignore"):
            if (ma == 0 and abs(np.log(f32(ra))) > 1.5) or (mb == 0 and abs(f32(rb)) > 200):
                out["branches"].add("relative_affine_out_of_range")
                return out
        if ma < 0:
            out["aff"][0] = 0.0
        if mb < 0:
            out["aff"][1] = 0.0
        out["ok"] = True
        return out


def flow_bound(res):
    """for rs[2 .. 4] of a calc_res: n 2^-53 sum|term| over the divisor, and one rounding of the quotient"""
    a = res["abs"]
    with np.errstate(all="ignore"):
        return np.array([a["n_flow"] * 2.0 ** -53 * s / a["den"] + np.spacing(s / a["den"]) for s in (a["sT"], 0.0, a["sRT"])])


def se3_exp(xi):
    """sophus/se3.hpp:406-428 with so3.hpp:343-369, as a 4 x 4 matrix"""
    ups, om = np.asarray(xi[:3], dtype=np.float64), np.asarray(xi[3:], dtype=np.float64)
    th2 = float(om @ om)
    th = math.sqrt(th2)
    if th < 1e-10:
        imag, real = 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, 1.0 - 0.5 * th2 + th2 * th2 / 384.0
    else:
        imag, real = math.sin(0.5 * th) / th, math.cos(0.5 * th)
    q = np.array([imag * om[0], imag * om[1], imag * om[2], real])
    q = q / np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    V = R if th < 1e-10 else np.eye(3) + (1 - math.cos(th)) / th2 * Om + (th - math.sin(th)) / (th2 * th) * (Om @ Om)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, V @ ups
    return M


def same_bits(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        u = f"u{a.dtype.itemsize}"
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def open_case(c, **variant):
    o = Oracle(c.H, c.W, c.levels, c.K, c.prm, **variant)
    o.set_ref(c.ref, c.cp, c.hdif, c.exposure_ref, c.aff_ref)
    o.set_new(c.new, c.exposure_new)
    return o
