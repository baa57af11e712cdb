"""Seeded cases for the activation tests (tests/test_activate_oracle.py, tests/test_activate_gpu.py), all small, built on
immature_cases.py's scenes: a textured plane seen by F window frames at slightly different poses and four further frames along a
translating path.  Every host's points are created and traced on those four frames with np_immature_oracle first, so the intervals
the candidate rule and the fit read are real.  What the cases add on purpose:
  - frame 1 has a NaN patch and frame 2 a block of foreign texture (F >= 3; F = 8: every frame from 2 on, so that points there keep
    fewer than min_obs residuals IN): residuals go OOB at a late tap and OUTLIER;
  - w64_f3_frac's newest frame is 0.35 to the side, so that border points project outside the map; w64_f2's baseline is small enough
    for Hdd to fall on both sides of min_idepth_h_act;
  - w64: a 64 x 48 image (map 32 x 24) whose active points cover the map, with seeds at u1 = 1, u1 = w1 - 1 and v1 = h1 - 1;
  - corner: a 256 x 192 image (map 128 x 96) whose active points sit in one corner, so cells beyond 39 rounds keep 1000;
  - F in {2, 3, 8, 10}, n_active = 0, a host without points, gn_its 0 and 3, min_obs 1 and 3, current_min_act_dist 0 and 4, and 1.5 (w64_f3_frac): with a whole threshold the
    fraction ptp0 - floorf(ptp0) never decides;
  - pre0: the precalc of slightly different poses (a non-zero linearisation offset), for the PRE_RTll_0 mutation."""
import numpy as np

import immature_cases as ic
import np_activate_oracle as ao
import np_immature_oracle as no

F = np.float32


def level1(K4):
    """K[1] of CoarseDistanceMap::makeK"""
    fx, fy, cx, cy = K4
    return np.array([[fx * 0.5, 0, (cx + 0.5) / 2 - 0.5], [0, fy * 0.5, (cy + 0.5) / 2 - 0.5], [0, 0, 1]], dtype=F)


def distance_precalc(K4, R, t):
    fx, fy, cx, cy = K4
    K0 = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)
    Ki0 = np.linalg.inv(K0).astype(F)
    K1 = level1(K4)
    return ((K1 @ np.asarray(R, dtype=F)) @ Ki0).astype(F), (K1 @ np.asarray(t, dtype=F)).astype(F)


def relative(poses, h, t):
    (Rh, ph), (Rt, pt) = poses[h], poses[t]
    return Rt.T @ Rh, Rt.T @ (ph - pt)


def precalc(poses, aff_step=(0.01, -0.3)):
    n = len(poses)
    pre = np.zeros((n, n, 14), F)
    for h in range(n):
        for t in range(n):
            R, tr = relative(poses, h, t)
            pre[h, t, :9] = np.asarray(R, F).ravel()
            pre[h, t, 9:12] = np.asarray(tr, F)
            pre[h, t, 12:] = (1.0 + aff_step[0] * (t - h), aff_step[1] * (t - h))
    return pre


class Case:
    pass


def make_case(name, seed, H, W, K4, counts, base, path, n_active, act_prm, min_dist, flagged=None, corner=False, cover=False, newest_shift=0.0):
    sc = ic.Scene(seed, H, W, K4)
    rng = sc.rng
    c = Case()
    c.name, c.H, c.W, c.K4, c.F, c.act_prm, c.min_dist = name, H, W, K4, len(counts), act_prm, float(min_dist)
    c.newest = c.F - 1
    c.flagged = np.zeros(c.F, np.uint8) if flagged is None else np.asarray(flagged, np.uint8)
    c.poses, c.images, c.hosts = [], [], []
    for h, n in enumerate(counts):
        R = ic.rot(*(rng.uniform(-0.015, 0.015, 2)), rng.uniform(-0.04, 0.04))
        p = np.append(rng.uniform(-base, base, 2), rng.uniform(-base, base) * 0.5)
        if h == len(counts) - 1:
            p[0] += newest_shift                      # a newest frame far enough for border points to leave the map
        c.poses.append((R, p))
        img = sc.render(R, p)
        if c.F >= 3 and h == 1:
            img[H // 5:H // 5 + 7, W // 6:W // 6 + 9] = np.nan
        if c.F >= 3 and (h == 2 or (c.F == 8 and h > 2)):
            yy, xx = np.mgrid[0:H, 0:W]
            y0, x0 = H // 2, W // 2
            img[y0:y0 + 12, x0:x0 + 16] = (128 + 100 * np.sin(2.1 * xx) * np.cos(1.7 * yy))[y0:y0 + 12, x0:x0 + 16].astype(F)
        c.images.append(img)
        c.hosts.append(dict(uv=ic._points(rng, H, W, n, 4), type=rng.choice([1.0, 2.0, 4.0], n).astype(F)))
    # the traces that give the intervals: four frames along the path
    prm = no.params()
    c.imm_prm = {}
    himg = [no.make_image(im) for im in c.images]
    c.P = [no.construct(himg[h], c.hosts[h]["uv"], c.hosts[h]["type"], None, None, prm) for h in range(c.F)]
    c.trace_targets, c.trace_steps = [], []
    for k in range(4):
        Rt = ic.rot(*(rng.uniform(-0.01, 0.01, 2)), rng.uniform(-0.03, 0.03))
        pt = np.asarray(path, dtype=np.float64) * (k + 1)
        c.trace_targets.append(sc.render(Rt, pt))
        timg = no.make_image(c.trace_targets[-1])
        c.trace_steps.append([])
        for h, (Rh, ph) in enumerate(c.poses):
            KRKi, Kt, a = ic.precalc32(K4, Rt.T @ Rh, Rt.T @ (ph - pt), (1.0 + 0.01 * k, -0.5 * k))
            no.trace(c.P[h], timg, KRKi, Kt, a, prm)
            c.trace_steps[-1].append((KRKi, Kt, a))
    c.himg = himg
    # host -> newest at level 1
    c.KRKi1, c.Kt1 = np.zeros((c.F, 3, 3), F), np.zeros((c.F, 3), F)
    for h in range(c.F):
        c.KRKi1[h], c.Kt1[h] = distance_precalc(K4, *relative(c.poses, h, c.newest))
    # the active points, grouped by host (some hosted by `newest`: skipped)
    w1, h1 = W >> 1, H >> 1
    rows = []
    if n_active:
        per = max(1, n_active // c.F)
        for h in range(c.F):
            if corner:
                uv = np.stack([rng.uniform(6, W * 0.12, per), rng.uniform(6, H * 0.12, per)], axis=1)
            else:
                uv = np.stack([rng.uniform(3, W - 3, per), rng.uniform(3, H - 3, per)], axis=1)
            for u, v in uv:
                rows.append((h, F(u), F(v), F(0.5 * (1 + 0.05 * rng.standard_normal()))))
        if cover:                                     # seeds on the ring and next to it, found by projecting host 0's pixels
            want = {"u1=1": lambda a, b: a == 1, "u1=w1-1": lambda a, b: a == w1 - 1, "v1=h1-1": lambda a, b: b == h1 - 1}
            extra = []
            for key, ok in want.items():
                for u in range(W):
                    for v in (H // 2, H - 2, H - 1):
                        cell, _ = ao._cell(c.KRKi1[0], c.Kt1[0], F(u), F(v), F(0.5), w1, h1)
                        if cell is not None and ok(*cell):
                            extra.append((0, F(u), F(v), F(0.5)))
                            break
                    else:
                        continue
                    break
            rows = [r for r in rows if r[0] == 0] + extra + [r for r in rows if r[0] != 0]
    c.active_host = np.array([r[0] for r in rows], np.int32)
    c.active = np.array([r[1:] for r in rows], F).reshape(-1, 3)
    c.pre = precalc(c.poses)
    moved = [(ic.rot(*(rng.uniform(-0.004, 0.004, 3))) @ R, p + rng.uniform(-0.004, 0.004, 3)) for R, p in c.poses]
    c.pre0 = precalc(moved)
    return c


_CASES = None


def cases():
    """name -> Case, built once"""
    global _CASES
    if _CASES is None:
        KS, KM, KL = (55.0, 52.0, 33.5, 22.25), (82.0, 77.0, 50.5, 33.25), (210.0, 200.0, 130.5, 93.25)
        cs = [
            make_case("w64_f3", 21, 48, 64, KS, [160, 120, 40], 0.03, (0.02, 0.004, 0.003), 90, dict(), 4.0, cover=True),
            make_case("w64_f3_frac", 34, 48, 64, KS, [120, 80, 10], 0.03, (0.02, -0.004, 0.003), 12, dict(), 1.5, newest_shift=0.35),
            make_case("w64_f2_noactive", 22, 48, 64, KS, [200, 30], 0.007, (0.015, -0.01, 0.0), 0, dict(), 0.0),
            make_case("m96_f8_obs3", 45, 72, 96, KM, [60, 45, 0, 30, 50, 40, 35, 15], 0.035, (0.02, 0.006, 0.002), 30, dict(min_obs=3), 0.0,
                      flagged=[0, 1, 0, 0, 0, 0, 0, 0]),
            make_case("corner_f3_gn0", 24, 192, 256, KL, [256, 200, 20], 0.03, (0.02, 0.0, 0.0), 60, dict(gn_its_on_point_activation=0), 4.0,
                      corner=True),
            make_case("m96_f10", 57, 72, 96, KM, [24, 20, 16, 24, 20, 16, 24, 20, 16, 8], 0.03, (-0.01, 0.02, 0.002), 100, dict(), 0.0),
        ]
        _CASES = {c.name: c for c in cs}
    return _CASES


# The seeds are chosen so that, on the oracle alone, no comparison is within 4 ulps of its threshold.  A Gauss-Newton step that has
# converged leaves E' within a few ulps of E, so a case with several hundred fitted points nearly always holds one: the two cases
# with many frames keep their hosts small.
_ORACLE = {}


def oracle_run(name, **variant):
    """The oracle over a whole case, once per (case, variant), never modified by the tests: the map after seeding and after the
    selection, the fates after the selection and after the fit, the fit's results, the points afterwards and the statistics.
    variant: the mutations of np_activate_oracle plus pre0 (the fit reads the precalc of the moved poses)."""
    key = (name,) + tuple(sorted(variant.items()))
    if key not in _ORACLE:
        c = cases()[name]
        prm = ao.params(**c.act_prm)
        v = dict(variant)
        bfs = {k: v.pop(k) for k in ("rounds", "even8", "expand_ring") if k in v}
        sel = {k: v.pop(k) for k in ("reverse_hosts", "div_floor") if k in v}
        pre = c.pre0 if v.pop("pre0", False) else c.pre
        w1, h1 = c.W >> 1, c.H >> 1
        m = ao.make_distance_map(w1, h1, c.newest, c.KRKi1, c.Kt1, c.active_host, c.active, **bfs)
        seeded = ao.map_array(m, w1, h1)
        P = [no.copy_points(p) for p in c.P]
        fates, und = ao.select(P, c.newest, c.KRKi1, c.Kt1, c.flagged, c.min_dist, prm, m, w1, h1, **sel, **bfs)
        selected = ao.map_array(m, w1, h1)
        fates_sel = [f.copy() for f in fates]
        results, st = ao.optimize(P, fates, c.himg, c.K4, pre, prm, no.params()["huber_th"], **v)
        st["undecided"] += und
        _ORACLE[key] = dict(prm=prm, map_seeded=seeded, map_selected=selected, fates_selected=fates_sel, fates=fates, results=results, points=P, stats=st)
    return _ORACLE[key]
