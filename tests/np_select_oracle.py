"""DSO's pixel selector in its LITERAL form: makeImages with absSquaredGrad, makeHists, select as the nested loop over 4 pot blocks,
2 pot blocks, pot cells and pixels with a running n2, and makeMaps with its recursion — numpy float32, written from the reference
(src/mapping/PixelSelector.cpp, src/tracking/HessianBlocks.cpp:139-202) independently of csrc/eds_pixsel.hpp, which states select in
its scan form: the two formulations check each other.

Elementwise arithmetic (thresholds, dirNorm under each of the 16 directions) is formed for the whole image at once in float32, which
rounds as the scalar expression does; every DECISION is taken in the loop, in the reference's order.  `mut` switches on one of the
deliberate mistakes the tests use to show that the cases discriminate.  `stats` counts the branches taken and the comparisons that a
4-ulp error could decide the other way."""
import numpy as np

f32 = np.float32
DIRECTIONS = np.array([(0, 1.0000), (0.3827, 0.9239), (0.1951, 0.9808), (0.9239, 0.3827), (0.7071, 0.7071), (0.3827, -0.9239), (0.8315, 0.5556),
                       (0.8315, -0.5556), (0.5556, -0.8315), (0.9808, 0.1951), (0.9239, -0.3827), (0.7071, -0.7071), (0.5556, 0.8315),
                       (0.9808, -0.1951), (1.0000, 0.0000), (0.1951, -0.9808)], dtype=np.float64).astype(np.float32)
MUTATIONS = ("raster_tiebreak", "dw2_no_quirk", "clamp32_everywhere", "rn_per_pixel", "ge", "n2_per_block")


def params(**over):
    p = dict(min_grad_hist_cut=0.5, min_grad_hist_add=7.0, grad_downweight_per_level=0.75, select_direction_distribution=1)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def _ulps(a, b):
    """distance in float32 steps between two non-negative finite float32 arrays"""
    return np.abs(np.asarray(a, f32).view(np.int32).astype(np.int64) - np.asarray(b, f32).view(np.int32).astype(np.int64))


def make_images(image, B=None):
    """levels 0 .. 2 as h x w x (colour, dx, dy, absSquaredGrad)"""
    out = []
    c = np.ascontiguousarray(image, dtype=f32)
    with np.errstate(all="ignore"):
        for lvl in range(3):
            if lvl > 0:
                p = out[-1][:, :, 0]
                h, w = p.shape[0] >> 1, p.shape[1] >> 1
                c = f32(0.25) * (((p[0:2 * h:2, 0:2 * w:2] + p[0:2 * h:2, 1:2 * w:2]) + p[1:2 * h:2, 0:2 * w:2]) + p[1:2 * h:2, 1:2 * w:2])
            h, w = c.shape
            flat = c.reshape(-1)
            dx, dy, ag = np.zeros(h * w, f32), np.zeros(h * w, f32), np.zeros(h * w, f32)
            i = np.arange(w, w * (h - 1))
            gx = f32(0.5) * (flat[i + 1] - flat[i - 1])
            gy = f32(0.5) * (flat[i + w] - flat[i - w])
            gx[~np.isfinite(gx)] = 0
            gy[~np.isfinite(gy)] = 0
            a = gx * gx + gy * gy
            if B is not None:
                Bt = np.asarray(B, f32)
                t = flat[i] + f32(0.5)
                ci = np.where(~(t >= 5), 5, np.where(~(t < 250), 250, np.nan_to_num(t, nan=5.0, posinf=250.0, neginf=5.0).clip(0, 300).astype(np.int64)))
                gw = Bt[ci + 1] - Bt[ci]
                a = a * (gw * gw)
            dx[i], dy[i], ag[i] = gx, gy, a
            out.append(np.stack([flat, dx, dy, ag], axis=-1).reshape(h, w, 4).astype(f32))
    return out


def hist_quantil(hist, below):
    th = int(f32(hist[0]) * f32(below) + f32(0.5))
    for i in range(90):
        th -= int(hist[i + 1])
        if th < 0:
            return i
    return 90


def make_hists(ag0, prm):
    h, w = ag0.shape
    w32, h32 = w // 32, h // 32
    ths, ths_s = np.zeros((h32, w32), f32), np.zeros((h32, w32), f32)
    for y in range(h32):
        for x in range(w32):
            hist = np.zeros(100, np.int64)              # bins past 49 are never filled: 0 (defined behaviour 5)
            for j in range(32):
                for i in range(32):
                    it, jt = i + 32 * x, j + 32 * y
                    if it > w - 2 or jt > h - 2 or it < 1 or jt < 1:
                        continue
                    with np.errstate(all="ignore"):
                        r = np.sqrt(ag0[jt, it])
                    g = 48 if not (r < 49) else min(int(r), 48)
                    hist[g + 1] += 1
                    hist[0] += 1
            ths[y, x] = f32(hist_quantil(hist, prm["min_grad_hist_cut"])) + f32(prm["min_grad_hist_add"])
    for y in range(h32):
        for x in range(w32):
            s, num = f32(0), f32(0)
            if x > 0:
                if y > 0:
                    num += f32(1); s += ths[y - 1, x - 1]
                if y < h32 - 1:
                    num += f32(1); s += ths[y + 1, x - 1]
                num += f32(1); s += ths[y, x - 1]
            if x < w32 - 1:
                if y > 0:
                    num += f32(1); s += ths[y - 1, x + 1]
                if y < h32 - 1:
                    num += f32(1); s += ths[y + 1, x + 1]
                num += f32(1); s += ths[y, x + 1]
            if y > 0:
                num += f32(1); s += ths[y - 1, x]
            if y < h32 - 1:
                num += f32(1); s += ths[y + 1, x]
            num += f32(1); s += ths[y, x]
            ths_s[y, x] = (s / num) * (s / num)
    return ths, ths_s


def _pixel_thresholds(w, h, ths_s, mut, stats):
    """thsSmoothed[(xf >> 5) + (yf >> 5) * thsStep] per pixel, with defined behaviour 1"""
    h32, w32 = ths_s.shape
    flat_t = ths_s.reshape(-1)
    th = np.zeros((h, w), f32)
    for yf in range(h):
        for xf in range(w):
            k = (xf >> 5) + (yf >> 5) * w32
            clamped = min(xf >> 5, w32 - 1) + min(yf >> 5, h32 - 1) * w32
            used = not (xf < 4 or xf >= w - 5 or yf < 4 or yf > h - 4)
            if mut == "clamp32_everywhere":
                k = clamped
            elif k >= w32 * h32:
                k = clamped
                stats["ths_clamped"] = stats.get("ths_clamped", 0) + used
            elif (xf >> 5) >= w32:
                stats["ths_aliased"] = stats.get("ths_aliased", 0) + used
            th[yf, xf] = flat_t[k]
    return th


def select(L, ths_s, table, pot, th_factor, prm, mut=None, stats=None):
    """the nested loop of :231-374; returns the map (h x w uint8) and (n2, n3, n4)"""
    stats = {} if stats is None else stats
    h, w = L[0].shape[:2]
    w1, w2 = L[1].shape[1], L[2].shape[1]
    thf = f32(th_factor)
    dw1 = f32(prm["grad_downweight_per_level"])
    dw2 = dw1 * dw1
    dist = int(prm["select_direction_distribution"])
    with np.errstate(all="ignore"):
        TH0 = _pixel_thresholds(w, h, ths_s, mut, stats)
        TH1 = TH0 * dw1
        TH2 = (TH0 * dw2) if mut == "dw2_no_quirk" else (TH1 * dw2)
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        i1 = (xs.astype(f32) * f32(0.5) + f32(0.25)).astype(np.int64) + (ys.astype(f32) * f32(0.5) + f32(0.25)).astype(np.int64) * w1
        i2 = ((xs.astype(f32) * f32(0.25)).astype(np.float64) + 0.125).astype(np.int64) + ((ys.astype(f32) * f32(0.25)).astype(np.float64) + 0.125).astype(np.int64) * w2
        inside = ~((xs < 4) | (xs >= w - 5) | (ys < 4) | (ys > h - 4))
        i1 = np.where(inside, i1, 0)
        i2 = np.where(inside, i2, 0)
        AG0 = L[0][:, :, 3]
        AG1 = L[1][:, :, 3].reshape(-1)[i1]
        AG2 = L[2][:, :, 3].reshape(-1)[i2]
        T0, T1, T2 = TH0 * thf, TH1 * thf, TH2 * thf
        gx, gy = L[0][:, :, 1], L[0][:, :, 2]
        DN = np.stack([np.abs(gx * DIRECTIONS[d, 0] + gy * DIRECTIONS[d, 1]) for d in range(16)])
        for a, t in ((AG0, T0), (AG1, T1), (AG2, T2)):
            ok = inside & np.isfinite(a) & np.isfinite(t) & (a >= 0) & (t >= 0)
            stats["undecided_ag"] = stats.get("undecided_ag", 0) + int(np.count_nonzero(_ulps(np.where(ok, a, 0), np.where(ok, t, 1e30)) <= 4))
        C0, C1, C2 = (AG0 > T0).reshape(-1).tolist(), (AG1 > T1).reshape(-1).tolist(), (AG2 > T2).reshape(-1).tolist()
    ag0, ag1, ag2 = AG0.reshape(-1).tolist(), AG1.reshape(-1).tolist(), AG2.reshape(-1).tolist()
    dn = [DN[d].reshape(-1).tolist() for d in range(16)]
    ge = mut == "ge"
    raster = mut == "raster_tiebreak"

    def better(v, best, idx, best_idx):
        if best > 0 and v != best and v > 0 and abs(v - best) <= 6e-7 * best and _ulps(v, best) <= 4:
            stats["undecided_dirnorm"] = stats.get("undecided_dirnorm", 0) + 1
        if v == best and best > 0 and best_idx >= 0:
            stats["dirnorm_ties"] = stats.get("dirnorm_ties", 0) + 1
            if raster:
                return idx < best_idx
        return v >= best if ge else v > best

    tab = [int(t) & 0xF for t in np.asarray(table).reshape(-1)]
    out = np.zeros(h * w, np.uint8)
    n2 = n3 = n4 = 0
    for y4 in range(0, h, 4 * pot):
        for x4 in range(0, w, 4 * pot):
            my3, mx3 = min(4 * pot, h - y4), min(4 * pot, w - x4)
            bestIdx4, bestVal4 = -1, 0.0
            nb = 0                                      # the n2_per_block mutation counts from the block's start
            dir4 = tab[nb if mut == "n2_per_block" else n2]
            for y3 in range(0, my3, 2 * pot):
                for x3 in range(0, mx3, 2 * pot):
                    x34, y34 = x3 + x4, y3 + y4
                    my2, mx2 = min(2 * pot, h - y34), min(2 * pot, w - x34)
                    bestIdx3, bestVal3 = -1, 0.0
                    dir3 = tab[nb if mut == "n2_per_block" else n2]
                    for y2 in range(0, my2, pot):
                        for x2 in range(0, mx2, pot):
                            x234, y234 = x2 + x34, y2 + y34
                            my1, mx1 = min(pot, h - y234), min(pot, w - x234)
                            bestIdx2, bestVal2 = -1, 0.0
                            dir2 = tab[nb if mut == "n2_per_block" else n2]
                            for y1 in range(my1):
                                for x1 in range(mx1):
                                    xf, yf = x1 + x234, y1 + y234
                                    idx = xf + w * yf
                                    if xf < 4 or xf >= w - 5 or yf < 4 or yf > h - 4:
                                        continue
                                    if C0[idx]:
                                        v = dn[dir2][idx] if dist else ag0[idx]
                                        if better(v, bestVal2, idx, bestIdx2):
                                            bestVal2, bestIdx2, bestIdx3, bestIdx4 = v, idx, -2, -2
                                    if bestIdx3 == -2:
                                        continue
                                    if C1[idx]:
                                        v = dn[dir3][idx] if dist else ag1[idx]
                                        if better(v, bestVal3, idx, bestIdx3):
                                            bestVal3, bestIdx3, bestIdx4 = v, idx, -2
                                    if bestIdx4 == -2:
                                        continue
                                    if C2[idx]:
                                        v = dn[dir4][idx] if dist else ag2[idx]
                                        if better(v, bestVal4, idx, bestIdx4):
                                            bestVal4, bestIdx4 = v, idx
                            if bestIdx2 > 0:
                                out[bestIdx2] = 1
                                bestVal3 = 1e10
                                n2 += 1
                                nb += 1
                    if bestIdx3 > 0:
                        out[bestIdx3] = 2
                        bestVal4 = 1e10
                        n3 += 1
            if bestIdx4 > 0:
                out[bestIdx4] = 4
                n4 += 1
    return out.reshape(h, w), (n2, n3, n4)


def ideal_potential(f):
    """(int)(sqrtf(K / numWant) - 1) with defined behaviour 3"""
    if not (f >= 1):
        return 1
    if not (f < 2.0 ** 30):
        return 1 << 30
    return int(f)


class Selector:
    """the reference's object: randomPattern, currentPotential, the histogram of the frame it saw last"""

    def __init__(self, H, W, table, **prm):
        self.H, self.W = H, W
        self.table = np.asarray(table, np.uint8).reshape(-1)
        self.prm = params(**prm)
        self.potential = 3
        self.L = None
        self.hist_frame = None
        self.stats = {}

    def set_image(self, image, B=None):
        self.L = make_images(image, B)
        self.frame = object()

    def make_maps(self, density, recursions_left, th_factor=1.0, mut=None):
        """returns dict(num_have_sub, map, passes [(potential, n2, n3, n4)], pass_maps, potential)"""
        passes, pass_maps = [], []
        st = self.stats
        while True:
            if self.hist_frame is not self.frame:
                self.ths, self.ths_s = make_hists(self.L[0][:, :, 3], self.prm)
                self.hist_frame = self.frame
                st["make_hists"] = st.get("make_hists", 0) + 1
            m, n = select(self.L, self.ths_s, self.table, min(self.potential, max(self.H, self.W)), th_factor, self.prm, mut, st)
            passes.append((self.potential,) + tuple(n))
            pass_maps.append(m.copy())
            with np.errstate(all="ignore"):
                numHave = f32(n[0] + n[1] + n[2])
                numWant = f32(density)
                quotia = numWant / numHave
                K = numHave * f32(self.potential + 1) * f32(self.potential + 1)
                ideal = ideal_potential(np.sqrt(K / numWant) - f32(1))
            q = float(quotia)
            for edge in (0.25, 0.95, 1.25):
                if np.isfinite(q) and q != edge and _ulps(f32(q), f32(edge)) <= 4:
                    st["undecided_quotia"] = st.get("undecided_quotia", 0) + 1
            if recursions_left > 0 and q > 1.25 and self.potential > 1:
                if ideal >= self.potential:
                    ideal = self.potential - 1
                self.potential = ideal
                recursions_left -= 1
                st["recurse_smaller"] = st.get("recurse_smaller", 0) + 1
                continue
            if recursions_left > 0 and q < 0.25:
                if ideal <= self.potential:
                    ideal = self.potential + 1
                self.potential = ideal
                recursions_left -= 1
                st["recurse_larger"] = st.get("recurse_larger", 0) + 1
                continue
            num_have_sub = int(numHave)
            flat = m.reshape(-1)
            if q < 0.95:
                char_th = int(f32(255) * quotia) & 0xFF
                rn = 0
                for i in range(flat.size):
                    if flat[i] != 0:
                        if self.table[rn] > char_th:
                            flat[i] = 0
                            num_have_sub -= 1
                            st["sub_removed"] = st.get("sub_removed", 0) + 1
                        rn += 1
                    elif mut == "rn_per_pixel":
                        rn += 1
                st["subselect"] = st.get("subselect", 0) + 1
            else:
                st["no_subselect"] = st.get("no_subselect", 0) + 1
            self.potential = ideal
            for v in (1, 2, 4):
                st[f"map_{v}"] = st.get(f"map_{v}", 0) + int(np.count_nonzero(flat == v))
            ys, xs = np.nonzero(m)
            return dict(num_have_sub=num_have_sub, map=m, passes=passes, pass_maps=pass_maps, potential=self.potential,
                        uv=np.stack([xs, ys], axis=1).astype(np.int32), type=m[ys, xs].astype(np.float32))
