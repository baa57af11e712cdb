"""numpy float32 restatement of the activation of DSO's immature points (include/eds_hip_activate.h).  Written from the reference text
for the callees — CoarseDistanceMap::makeDistanceMap, growDistBFS and addIntoDistFinal (src/tracking/CoarseTracker.cpp:731-882),
ImmaturePoint::linearizeResidual (src/tracking/ImmaturePoint.cpp:529-596), projectPoint and derive_idepth
(src/tracking/ResidualProjections.h:35-86) — and from the header's statement for the two loops that drive them, independently of
csrc/eds_activate.hpp.  growDistBFS is the LITERAL list form of lines 779-873 (two lists, cells appended as they are set), not the
round form the kernels run, so that the two are checked against each other.

Every array is float32 and every operation one IEEE operation in the reference's order.  The switches of `grow`, `select` and
`optimize` are NOT the reference: they are mutations the tests use to show that their cases tell them apart."""
import numpy as np

import np_immature_oracle as no

F = np.float32
GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
ST_IN, ST_OOB, ST_OUTLIER = 0, 1, 2
NONE, DELETED_UNTRACED, DELETED_CANNOT, KEPT_CANNOT, DELETED_OUT_OF_MAP, CHOSEN, KEPT_TOO_CLOSE, KEPT_WEAK, DROPPED, ACTIVATED = range(10)
FATE_NAMES = ("NONE", "DELETED_UNTRACED", "DELETED_CANNOT", "KEPT_CANNOT", "DELETED_OUT_OF_MAP", "CHOSEN", "KEPT_TOO_CLOSE", "KEPT_WEAK", "DROPPED",
              "ACTIVATED")
DEFAULTS = dict(min_idepth_h_act=100.0, gn_its_on_point_activation=3, min_trace_quality=3.0, max_trace_pixel_interval=8.0, min_obs=1,
                scale_idepth=1.0)
_INT = ("gn_its_on_point_activation", "min_obs")
N4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
N8 = N4 + ((1, 1), (-1, 1), (-1, -1), (1, -1))


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return {k: (int(v) if k in _INT else F(v)) for k, v in p.items()}


def grow(m, w1, h1, lst, rounds=40, even8=False, expand_ring=False):
    """growDistBFS(len(lst)) on the flat list of ints m, with bfsList1 = lst"""
    for k in range(1, rounds):
        cur, lst = lst, []
        nb = N8 if (k % 2 == 1 or even8) else N4
        for x, y in cur:
            if not expand_ring and (x == 0 or y == 0 or x == w1 - 1 or y == h1 - 1):
                continue
            for dx, dy in nb:
                nx, ny = x + dx, y + dy
                if expand_ring and (nx < 0 or ny < 0 or nx >= w1 or ny >= h1):
                    continue                      # the mutation must not index outside the map
                j = nx + ny * w1
                if m[j] > k:
                    m[j] = k
                    lst.append((nx, ny))


def _cell(K, Kt, u, v, idp, w1, h1):
    """the cell of ptp = KRKi (u, v, 1) + Kt idepth, or None; and ptp"""
    with np.errstate(all="ignore"):
        p = [K[i, 0] * u + K[i, 1] * v + K[i, 2] * F(1) + Kt[i] * idp for i in range(3)]
        qu, qv = p[0] / p[2], p[1] / p[2]
        if not (np.abs(qu) <= F(1048576.0) and np.abs(qv) <= F(1048576.0)):
            return None, p
        u1, v1 = int(qu + F(0.5)), int(qv + F(0.5))
    if not (u1 > 0 and v1 > 0 and u1 < w1 and v1 < h1):
        return None, p
    return (u1, v1), p


def make_distance_map(w1, h1, newest, KRKi1, Kt1, active_host, active, **mut):
    """makeDistanceMap: the map as a flat list of ints (1000: never reached)"""
    K, T = np.asarray(KRKi1, F).reshape(-1, 3, 3), np.asarray(Kt1, F).reshape(-1, 3)
    active = np.asarray(active, F).reshape(-1, 3)
    m = [1000] * (w1 * h1)
    lst = []
    for i, h in enumerate(np.asarray(active_host, np.int64)):
        if h == newest:
            continue
        c, _ = _cell(K[h], T[h], active[i, 0], active[i, 1], active[i, 2], w1, h1)
        if c is None:
            continue
        m[c[0] + w1 * c[1]] = 0
        lst.append(c)
    grow(m, w1, h1, lst, **mut)
    return m


def map_array(m, w1, h1):
    return np.asarray(m, F).reshape(h1, w1)


def _near(a, b):
    """a comparison of a with b that 4 ulps could turn"""
    with np.errstate(all="ignore"):
        return bool(np.isfinite(a) and np.isfinite(b) and np.abs(F(a) - F(b)) <= F(4) * np.spacing(np.abs(F(b))))


def select(Ps, newest, KRKi1, Kt1, flagged, min_dist, prm, m, w1, h1, reverse_hosts=False, div_floor=False, **mut):
    """the candidate rule over the point sets Ps (one per host); m is modified.  Returns the fates per host and the undecided count."""
    K, T = np.asarray(KRKi1, F).reshape(-1, 3, 3), np.asarray(Kt1, F).reshape(-1, 3)
    fates = [np.zeros(len(P["u"]), np.int32) for P in Ps]
    undecided = 0
    order = range(len(Ps) - 1, -1, -1) if reverse_hosts else range(len(Ps))
    md = F(min_dist)
    for h in order:
        if h == newest:
            continue
        P = Ps[h]
        with np.errstate(all="ignore"):
            ssum = P["idepth_max"] + P["idepth_min"]
        for i in range(len(P["u"])):
            if not P["alive"][i]:
                continue
            st = P["status"][i]
            if not np.isfinite(P["idepth_max"][i]) or st == OUTLIER:
                fates[h][i] = DELETED_UNTRACED
                continue
            can = (st in (GOOD, SKIPPED, BADCONDITION, OOB) and P["last_interval"][i] < prm["max_trace_pixel_interval"] and
                   P["quality"][i] > prm["min_trace_quality"] and ssum[i] > 0)
            if not can:
                fates[h][i] = DELETED_CANNOT if (flagged[h] or st == OOB) else KEPT_CANNOT
                continue
            c, p = _cell(K[h], T[h], P["u"][i], P["v"][i], F(0.5) * ssum[i], w1, h1)
            if c is None:
                fates[h][i] = DELETED_OUT_OF_MAP
                continue
            with np.errstate(all="ignore"):
                q = p[0] / p[2] if div_floor else p[0]
                dist = F(m[c[0] + w1 * c[1]]) + (q - np.floor(q))
                th = md * P["type"][i]
            undecided += _near(dist, th)
            if dist >= th:
                fates[h][i] = CHOSEN
                m[c[0] + w1 * c[1]] = 0                    # addIntoDistFinal
                grow(m, w1, h1, [c], **mut)
            else:
                fates[h][i] = KEPT_TOO_CLOSE
    return fates, undecided


def _taps(P, idx, img_planes, H, W, K4, pre, idp, k, huber, scale):
    """tap k of linearizeResidual for the points idx of P at inverse depths idp: fail, and the addends to energyLeft, Hdd, bd"""
    fx, fy, cx, cy = (F(x) for x in K4)
    fxli, fyli = F(1) / fx, F(1) / fy
    R, t, aff = pre[:9], pre[9:12], pre[12:14]
    px, py = no.PATTERN[k]
    with np.errstate(all="ignore"):
        k0 = (P["u"][idx] + F(px) - cx) * fxli
        k1 = (P["v"][idx] + F(py) - cy) * fyli
        p0 = R[0] * k0 + R[1] * k1 + R[2] * F(1) + t[0] * idp
        p1 = R[3] * k0 + R[4] * k1 + R[5] * F(1) + t[1] * idp
        p2 = R[6] * k0 + R[7] * k1 + R[8] * F(1) + t[2] * idp
        dres = F(1) / p2
        fail = ~(dres > 0)
        u, v = p0 * dres, p1 * dres
        Ku, Kv = u * fx + cx, v * fy + cy
        fail |= ~((Ku > F(1.1)) & (Kv > F(1.1)) & (Ku < F(W - 3)) & (Kv < F(H - 3)))
        hc, hx, hy = no._interp(img_planes, W, H, np.where(fail, F(np.nan), Ku).astype(F), np.where(fail, F(np.nan), Kv).astype(F))
        fail |= ~np.isfinite(hc)
        r = hc - (aff[0] * P["color"][idx, k] + aff[1])
        hw = np.where(np.abs(r) < huber, F(1), huber / np.abs(r)).astype(F)
        w = P["weights"][idx, k]
        e = w * w * hw * r * r * (F(2) - hw)
        dxi, dyi = hx * fx, hy * fy
        d = (dxi * dres * (t[0] - t[2] * u) + dyi * dres * (t[1] - t[2] * v)) * scale
        hw = hw * (w * w)
        hh = (hw * d) * d
        bb = (hw * r) * d
    return fail, e.astype(F), hh.astype(F), bb.astype(F)


def optimize(Ps, fates, images, K4, pre, prm, huber, discard_partial=False, finite_on_new=False):
    """the fit of every CHOSEN point; Ps (alive) and fates are modified.  images: the window's frames as make_image gives them;
    pre: F x F x 14.  Returns per host a dict idepth, energy, hdd, bd, res_state, res_energy, and the statistics the tests assert."""
    nF = len(Ps)
    H, W, _ = images[0].shape
    planes = [[np.ascontiguousarray(im[..., c]).ravel() for c in range(3)] for im in images]
    pre = np.asarray(pre, F).reshape(nF, nF, 14)
    huber, scale, minH = F(huber), prm["scale_idepth"], prm["min_idepth_h_act"]
    st = dict(accept=0, reject=0, step_break=0, weak_first=0, weak_loop=0, dropped_few_in=0, oob_late_tap=0, outlier_slack1_only=0, undecided=0,
              finite_test_differs=0)
    out = []
    for h, P in enumerate(Ps):
        n = len(P["u"])
        res = dict(idepth=np.zeros(n, F), energy=np.zeros(n, F), hdd=np.zeros(n, F), bd=np.zeros(n, F),
                   res_state=np.full((n, nF), -1, np.int32), res_energy=np.zeros((n, nF), F))
        out.append(res)
        idx = np.flatnonzero(fates[h] == CHOSEN)
        m = len(idx)
        if m == 0:
            _retire(P, fates[h])
            continue
        targets = [t for t in range(nF) if t != h]
        R = len(targets)
        state, new_state = np.zeros((m, R), np.int32), np.zeros((m, R), np.int32)
        energy, new_energy = np.zeros((m, R), F), np.zeros((m, R), F)
        eth = P["energyTH"][idx]

        def ev(idp, slack, run):
            E, Hdd, bd = np.zeros(m, F), np.zeros(m, F), np.zeros(m, F)
            for r, t in enumerate(targets):
                go = state[:, r] != ST_OOB
                failed = np.zeros(m, bool)
                e = np.zeros(m, F)
                H0, b0 = Hdd.copy(), bd.copy()
                for k in range(8):
                    fail, ek, hk, bk = _taps(P, idx, planes[t], H, W, K4, pre[h, t], idp, k, huber, scale)
                    live = go & ~failed
                    ok = live & ~fail
                    st["oob_late_tap"] += int((live & fail & run).sum()) if k >= 1 else 0
                    with np.errstate(all="ignore"):
                        e = np.where(ok, e + ek, e).astype(F)
                        Hdd = np.where(ok, Hdd + hk, Hdd).astype(F)
                        bd = np.where(ok, bd + bk, bd).astype(F)
                    failed |= live & fail
                if discard_partial:
                    Hdd, bd = np.where(failed, H0, Hdd), np.where(failed, b0, bd)
                full = go & ~failed
                with np.errstate(all="ignore"):
                    th = eth * F(slack)
                    clamp = full & (e > th)
                    if slack == 1:
                        st["outlier_slack1_only"] += int((clamp & run & ~(e > eth * F(1000))).sum())
                    ne = np.where(clamp, th, e).astype(F)
                upd = run & full
                new_state[:, r] = np.where(run, np.where(full, np.where(clamp, ST_OUTLIER, ST_IN), ST_OOB), new_state[:, r])
                new_energy[:, r] = np.where(upd, ne, new_energy[:, r])
                ret = np.where(full, ne, energy[:, r])
                E = (E.astype(np.float64) + ret.astype(np.float64)).astype(F)
            return E, Hdd, bd

        def near(a, b):
            with np.errstate(all="ignore"):
                return np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= F(4) * np.spacing(np.abs(b)))

        with np.errstate(all="ignore"):
            idp = ((P["idepth_max"][idx] + P["idepth_min"][idx]) * F(0.5)).astype(F)
            run = np.ones(m, bool)
            E, Hdd, bd = ev(idp, 1000, run)
            state[:], energy[:] = new_state, new_energy
            fate = np.full(m, CHOSEN, np.int32)
            weak = ~np.isfinite(E) | (Hdd < minH)
            st["undecided"] += int(near(Hdd, np.full(m, minH, F)).sum())
            st["weak_first"] += int(weak.sum())
            fate[weak] = KEPT_WEAK
            run = ~weak
            lam = np.full(m, 0.1, F)
            for _ in range(prm["gn_its_on_point_activation"]):
                if not run.any():
                    break
                Hs = (Hdd * (F(1) + lam)).astype(F)
                step = ((1.0 / Hs.astype(np.float64)) * bd.astype(np.float64)).astype(F)
                nid = (idp - step).astype(F)
                E2, H2, b2 = ev(np.where(run, nid, idp).astype(F), 1, run)
                st["undecided"] += int((run & (near(H2, np.full(m, minH, F)) | near(E2, E))).sum())
                st["finite_test_differs"] += int((run & (np.isfinite(E) != np.isfinite(E2))).sum())
                weak = run & (~np.isfinite(E2 if finite_on_new else E) | (H2 < minH))
                st["weak_loop"] += int(weak.sum())
                fate[weak] = KEPT_WEAK
                run &= ~weak
                acc = run & (E2 < E)
                rej = run & ~acc
                st["accept"] += int(acc.sum())
                st["reject"] += int(rej.sum())
                idp, E, Hdd, bd = np.where(acc, nid, idp), np.where(acc, E2, E), np.where(acc, H2, Hdd), np.where(acc, b2, bd)
                state[acc], energy[acc] = new_state[acc], new_energy[acc]
                lam = np.where(acc, lam * F(0.5), np.where(rej, lam * F(5), lam)).astype(F)
                brk = run & (np.abs(step).astype(np.float64) < 0.0001 * idp.astype(np.float64))
                st["step_break"] += int(brk.sum())
                run &= ~brk
            done = fate == CHOSEN
            n_in = (state == ST_IN).sum(axis=1)
            few = done & np.isfinite(idp) & (n_in < prm["min_obs"])
            st["dropped_few_in"] += int(few.sum())
            drop = done & (~np.isfinite(idp) | (n_in < prm["min_obs"]))
            fate[drop] = DROPPED
            fate[done & ~drop] = ACTIVATED
        fates[h][idx] = fate
        res["idepth"][idx], res["energy"][idx], res["hdd"][idx], res["bd"][idx] = idp, E, Hdd, bd
        for r, t in enumerate(targets):
            res["res_state"][idx, t] = state[:, r]
            res["res_energy"][idx, t] = energy[:, r]
        _retire(P, fates[h])
    return out, st


def _retire(P, fate):
    leaves = (np.isin(fate, (ACTIVATED, DROPPED, DELETED_UNTRACED, DELETED_CANNOT, DELETED_OUT_OF_MAP)) | ((fate == KEPT_WEAK) & (P["status"] == OOB)))
    P["alive"] &= ~leaves


def activated(Ps, fates, results, scale=F(1)):
    """the arrays of eds_act_get_activated, in (host, index) order"""
    rows = [(h, i) for h in range(len(Ps)) for i in np.flatnonzero(fates[h] == ACTIVATED)]
    nF = len(Ps)
    o = dict(host=np.array([h for h, _ in rows], np.int32), index=np.array([i for _, i in rows], np.int32),
             uv=np.array([[Ps[h]["u"][i], Ps[h]["v"][i]] for h, i in rows], F).reshape(-1, 2), type=np.array([Ps[h]["type"][i] for h, i in rows], F),
             idepth=np.array([results[h]["idepth"][i] * scale for h, i in rows], F),
             color=np.array([Ps[h]["color"][i] for h, i in rows], F).reshape(-1, 8), weights=np.array([Ps[h]["weights"][i] for h, i in rows], F).reshape(-1, 8),
             target_mask=np.array([sum(1 << t for t in range(nF) if results[h]["res_state"][i, t] == ST_IN) for h, i in rows], np.uint64))
    return o
