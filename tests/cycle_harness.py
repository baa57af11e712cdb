"""One driver, two routes, for four keyframe cycles back to back on one set of handles over tests/cycle_cases.py.

``Driver("device")`` holds ``window.Window``, ``winsolve.WindowSolver``, ``winedit.WindowEdit``, ``winflag.WindowFlags``,
``immature.ImmaturePoints``, ``activate.Activation``, ``select.Selector`` and ``immdepth.ImmatureDepth``; fates, activated points, the
selection and the depth map stay on the device (``eds_wfl_*_flagged``, ``insert_activated(activation)``, ``create_points_selected``,
``map.seed_immature_from_window``).  With ``host_flags=True`` the same handles are fed the states, the fates, the selection and the
depth map read back and passed as host arrays: the entry points that existed before.  ``Driver("host")`` holds the g++ restatements
(``winsolve_harness.HostWindow`` / ``HostSolver``, ``winedit_harness.HostEdit``, the ``winflag_harness`` functions over arrays, the
activate, immature, select, immdepth and map harnesses), the arrays handed from one to the next here.

One cycle, in the order of INTEGRATION §3.16 / §3.17 (a snapshot after every numbered step):
 1  linearize with the cycle's precalc and thresholds; apply; every seventh residual is fixed (their linearized flags and res_toZeroF
    then travel through every later gather)
 2  two Gauss-Newton iterations: backup_idepths, solve, step_idepths, linearize, l_energy + m_energy; the step is accepted where the
    sum of the three energies fell (apply) and rejected otherwise (the backup restored, lambda raised); then eds_wed_set_state on
    the still valid state, so that deltaF follows the inverse depths as setDeltaF does.  The frames are not stepped: their poses
    stay the cycle's evaluation poses, the frames' step enters through the L and M energies alone
 3  linearize, apply_fixed(F, precalc, 0): the history's update.  The Hessians the flags read are those the last solve's point pass
    left: eds_win_point_hessians is not called, because the device's skips the linearized residuals and adds the L sums the solve
    left there, and the host window's restatement knows neither (its accumulate is only comparable without linearized residuals)
 4  remove_residuals(None)
 5  flag_points(F, 1 << leaving)
 6  marginalize_flagged(HM, bM)
 7  remove_flagged()
 8  marginalize_frame(leaving)
 9  set_frames(F - 1, the new keyframe); the eds_imm's hosts follow the window's slots.  An eds_imm has no entry point that removes a
    host, so every host above the leaving slot is created anew one index lower from its live points' pixels and takes their
    idepth_min / idepth_max / status through eds_map_set_immature_trace; both routes do exactly this
10  the new keyframe's immature points: the selector (the reference's random table) on its image, the depth map of the window's points
    moved into it (eds_map), the depth-seeded constructor (eds_imd) for the selected pixels
11  every host's immature points traced on the cycle's two in-between images
12  the activation: distance map from the window's points (read back for it on both routes), the candidate rule, the fit;
    insert_activated
13  set_state for the new F, insert_frame_residuals(F - 1)
On the device route the marks are probed where a running system would trip over a stale one: after step 7 the fates are stale, after
steps 12 and 13 eds_win_apply is EDS_ERR_STATE until the next linearize.
The device keeps two pairs of buffer sets.  The per-residual pair changes hands with every edit: five times a cycle.  The per-point
pair changes hands only in remove_flagged and insert_activated: twice a cycle, so every cycle's step 1 would find it on the same
side.  In cycles 2 and 4 a remove_points with all-zero flags follows step 4: it moves nothing and exchanges both pairs, so that at
step 1 the parity of each pair differs between the cycles (points 0, 0, 1, 1; residuals 0, 1, 1, 0)."""
import ctypes as C
import functools
import importlib

import numpy as np

import activate_harness as ah
import cycle_cases as cc
import harness_build as hb
import immature_harness as ih
import immdepth_harness as dh
import map_harness as mh
import np_activate_oracle as ao
import np_immature_oracle as no
import select_cases as sc
import select_harness as sh
import winedit_harness as weh
import winflag_harness as wfh
import winsolve_harness as wsh

MODE = wsh.DEFAULT_MODE
FIX_EVERY = 7
STEPS = 13


def _mod(name):
    return importlib.import_module("slam-eds_amd." + name)


@functools.lru_cache(maxsize=None)
def _table():
    return sc.reference_table(cc.H * cc.W)


class Driver:
    """the handles of one route, opened over the case's initial state"""

    def __init__(self, route, case=None, max_points=4096, max_residuals=16384, max_immature=1024, host_flags=False):
        assert route in ("device", "host")
        self.route, self.c, self.host_flags = route, case or cc.case(), host_flags
        self.caps = (int(max_points), int(max_residuals), int(max_immature))
        self.watch, self.before_insert = False, None                                                  # watch: the tables and the history are read right before every insert
        c = self.c
        if route == "device":
            self.w = _mod("window").Window(c.H, c.W, c.F, max_points=self.caps[0], max_residuals=self.caps[1])
            self.sv = _mod("winsolve").WindowSolver(self.w)
            self.ed = _mod("winedit").WindowEdit(self.w, self.sv)
            self.fl = _mod("winflag").WindowFlags(self.w)
            self.imm = _mod("immature").ImmaturePoints(c.H, c.W, c.F, self.caps[2], 2)
            self.act = _mod("activate").Activation(self.imm, *c.K4)
            self.sel = _mod("select").Selector(c.H, c.W, table=_table())
            self.imd = _mod("immdepth").ImmatureDepth(self.imm)
        else:
            self.w = wsh.HostWindow(c.H, c.W, c.F)
            self.sv = wsh.HostSolver(self.w)
            self.ed = weh.HostEdit(self.w)
            self.hl_imm, self.hl_act, self.hl_imd = ih.load_harness(), ah.load_harness(), dh.load_harness()
            self.sel = sh.HostSelector(c.H, c.W, table=_table())
            self.imm_prm, self.act_prm = no.params(), ao.params()
        self.w.set_calib(*c.K4)
        self.reset()

    def close(self):
        if self.route == "device":
            for x in (self.sel, self.imm, self.w):
                x.close()
        else:
            self.sel.close()
            self.sv.close()
            self.w.close()

    # ---- the initial state, on fresh handles or on used ones -------------------------------------------------------------------------------
    def reset(self):
        c, k = self.c, self.c.win
        self.ids = c.ids0
        self.fi = c.frame_inputs(self.ids)
        self.w.set_frames(0, self.fi.images)
        self.w.set_points(k.host, k.uv, k.color, k.weights, k.ids, k.idz)
        self.w.set_residuals(k.point, k.target, k.state, k.energy)
        self.HM, self.bM = c.HM.copy(), c.bM.copy()
        self.seeds = [dict(uv=s["uv"].copy(), type=s["type"].copy()) for s in c.immature]
        if self.route == "device":
            self.fl.set_history(**c.history)
            self.imm.set_host_images(0, self.fi.images)
            for h, s in enumerate(self.seeds):
                self.imm.create_points(h, s["uv"], s["type"])
            self.sel.potential = 3
        else:
            self.hist = {k: np.array(v) for k, v in c.history.items()}
            self.pts = [ih.construct(self.hl_imm, self.fi.images[h], s["uv"], s["type"], None, None, self.imm_prm) for h, s in enumerate(self.seeds)]
            self.sel.potential = 3
        f = self.fi
        self.sv.set_state(f.F, f.adH, f.adT, f.delta, f.prior, f.delta_prior, f.cPrior, f.cDelta, c.priorF, c.deltaF)
        self.valid = True
        self.exchanges = dict(points=0, residuals=0)                                                  # how often each set of buffers has changed hands: see exchanged()
        self.peaks = dict(points=self.w.n, residuals=self.w.m, immature=max(len(s["uv"]) for s in self.seeds))

    # ---- what a snapshot holds -------------------------------------------------------------------------------------------------------------
    def history(self):
        return self.fl.history() if self.route == "device" else {k: v.copy() for k, v in self.hist.items()}

    def immature_state(self):
        out = []
        for h in range(self.c.F):
            if self.route == "device":
                g, p = self.imm.get(h), self.imm.points(h)
                out.append(dict(idepth_min=g["idepth_min"], idepth_max=g["idepth_max"], quality=g["quality"], status=g["lastTraceStatus"],
                                last_uv=g["lastTraceUV"], last_interval=g["lastTracePixelInterval"], alive=p["alive"].astype(np.int32),
                                color=p["color"], weights=p["weights"], energyTH=p["energyTH"]))
            else:
                p = self.pts[h]
                out.append(dict(idepth_min=p["idepth_min"].copy(), idepth_max=p["idepth_max"].copy(), quality=p["quality"].copy(), status=p["status"].copy(),
                                last_uv=p["last_uv"].copy(), last_interval=p["last_interval"].copy(), alive=(p["alive"] != 0).astype(np.int32),
                                color=p["color"].copy(), weights=p["weights"].copy(), energyTH=p["energyTH"].copy()))
        return out

    def tables_and_history(self):
        w, ed = self.w, self.ed
        n, m, per_host = ed.counts()
        tables = weh.snapshot(w, self.sv, ed) if self.valid else dict(residuals=w.residuals(), points=w.points(), rows=ed.rows(state=False))
        return dict(tables=tables, counts=np.array([n, m, w.n, w.m], np.int32), per_host=per_host, history=self.history())

    def snapshot(self, cycle, step, **out):
        w, sv, ed = self.w, self.sv, self.ed
        if self.valid:
            tables = weh.snapshot(w, sv, ed)
        else:                                                                                          # between marginalize_frame and set_state
            n, m, per_host = ed.counts()
            assert (n, m) == (w.n, w.m)
            tables = dict(residuals=w.residuals(), points=w.points(), rows=ed.rows(state=False), counts=np.array([n, m], np.int32), per_host=per_host)
        snap = dict(cycle=cycle, step=step, tables=tables, history=self.history(), out=out, frames=tuple(self.ids))
        if step >= 9:
            snap["immature"] = self.immature_state()
        self.peaks["points"], self.peaks["residuals"] = max(self.peaks["points"], w.n), max(self.peaks["residuals"], w.m)
        return snap

    # ---- the steps that differ between the routes ------------------------------------------------------------------------------------------
    def _arrays(self):
        """the host route's (and the host-flag route's) view of the tables"""
        rows, res = self.ed.rows(state=False), self.w.residuals()
        return dict(host=rows["host"], uv=rows["uv"], point=rows["point"], target=rows["target"], state=res["state"], active=res["is_active"])

    def apply_fixed(self, f):
        if self.route == "device":
            return self.fl.apply_fixed(f.F, f.precalc, 0)
        self.w.apply(True)
        t = self._arrays()
        self.hist, counts = wfh.apply_fixed(self.hist, t["host"], t["uv"], self.sv.get(system=False)["idepth_scaled"], t["point"], t["target"], t["state"],
                                            t["active"], f.precalc, f.F, 0)
        return counts

    def exchanged(self, points):
        """An edit gathers into a second set of buffers and exchanges the sets.  The device keeps two pairs: the per-residual rows,
        which every edit exchanges, and the per-point rows (the points, their inverse depths, sums, solver rows and the history's
        point columns), which only eds_wed_remove_points and eds_wed_insert_activated exchange."""
        self.exchanges["residuals"] += 1
        self.exchanges["points"] += int(points)

    def remove_residuals(self):
        self.exchanged(points=False)
        if self.route == "device" and not self.host_flags:
            return self.ed.remove_residuals(None)
        t = self._arrays()
        sel = (t["state"] != 0).astype(np.int32)
        if self.route == "host":
            self.hist = wfh.remove_residuals(self.hist, t["point"], t["target"], sel == 0)
        return self.ed.remove_residuals(sel)

    def remove_no_points(self):
        """eds_wed_remove_points with all-zero flags: both pairs of buffers change hands and every row moves to where it was"""
        self.exchanged(points=True)
        if self.route == "host":
            self.hist = wfh.remove_points(self.hist, self._arrays()["point"], np.ones(self.w.n, bool))
        return self.ed.remove_points(np.zeros(self.w.n, np.int32))

    def flag_points(self, f, mask):
        if self.route == "device":
            totals, per_host = self.fl.flag_points(f.F, mask, f.precalc, f.th, **cc.FLAG_PARAMS)
            self.fates = self.fl.fates() if self.host_flags else None
            return np.concatenate([totals, per_host.ravel()])
        w, t = self.w, self._arrays()
        ids, hess = self.sv.get(system=False)["idepth_scaled"], w.points()["idepth_hessian"]
        self.fates, counts, cand = wfh.flag_points(self.hist, t["host"], ids, t["point"], t["target"], t["state"], hess, mask, prm=cc.FLAG_PARAMS)
        if w.m:                                                                                        # the candidates re-linearized: resetOOB, linearize, applyRes, fixLinearizationF
            self.ed.reset_oob(cand)
            pc, th = np.ascontiguousarray(f.precalc, np.float32), np.ascontiguousarray(f.th, np.float32)
            for p in np.flatnonzero(cand):
                w.L.win_linearize_points(w._h, f.F, hb.p(pc), hb.p(th), int(p), int(p) + 1)
            for p in np.flatnonzero(cand):
                w.L.win_apply_points(w._h, 1, int(p), int(p) + 1)
            self.sv.fix_linearization(((cand[t["point"]] != 0) & (w.residuals()["is_active"] != 0)).astype(np.int32))
        return counts

    def marginalize_flagged(self):
        if self.route == "device" and not self.host_flags:
            self.HM, self.bM, res_m = self.fl.marginalize_flagged(self.HM, self.bM)
        else:
            self.HM, self.bM, res_m = self.sv.marginalize_points((self.fates == 1).astype(np.int32), self.HM, self.bM)
        return res_m

    def remove_flagged(self):
        self.exchanged(points=True)
        if self.route == "device" and not self.host_flags:
            return self.fl.remove_flagged()
        if self.route == "host":
            self.hist = wfh.remove_points(self.hist, self._arrays()["point"], self.fates == 0)
        return self.ed.remove_points((self.fates != 0).astype(np.int32))

    def marginalize_frame(self, f, leaving):
        self.exchanged(points=False)
        if self.route == "host":
            t = self._arrays()
            self.hist = wfh.marginalize_frame(self.hist, t["point"], t["target"], leaving)
        self.HM, self.bM = self.ed.marginalize_frame(leaving, f.prior[leaving], f.delta_prior[leaving], self.HM, self.bM)
        self.valid = False

    def shift_immature_hosts(self, leaving, f):
        """step 9 for the immature points: see the module's docstring"""
        F = self.c.F
        state = self.immature_state()
        live = [s["alive"] != 0 for s in state]
        if self.route == "device":
            self.imm.set_host_images(0, f.images)
        else:
            self.pts.pop(leaving)
            self.pts.append(np.zeros(0, ih.POINT))
        self.seeds = [dict(uv=self.seeds[h]["uv"][live[h]], type=self.seeds[h]["type"][live[h]]) if h > leaving else self.seeds[h]
                      for h in range(F) if h != leaving] + [dict(uv=np.zeros((0, 2), np.int32), type=np.zeros(0, np.float32))]
        for old in range(leaving + 1, F):
            new, s, k = old - 1, self.seeds[old - 1], live[old]
            lo, hi, st = state[old]["idepth_min"][k], state[old]["idepth_max"][k], state[old]["status"][k]
            if self.route == "device":
                self.imm.create_points(new, s["uv"], s["type"])
                _mod("map").set_immature_trace(self.imm, new, lo, hi, st)
            else:
                p = ih.construct(self.hl_imm, f.images[new], s["uv"], s["type"], None, None, self.imm_prm)
                p["idepth_min"], p["idepth_max"], p["status"] = lo, hi, st
                self.pts[new] = p
        if self.route == "device":
            self.imm.create_points(F - 1, np.zeros((0, 2), np.int32), np.zeros(0, np.float32))

    def seed_new_keyframe(self, f):
        """step 10; returns (selected, points created, alive)"""
        c, F = self.c, self.c.F
        image = f.images[F - 1]
        rect = (3, 3, c.W - 5, c.H - 5)
        self.sel.set_image(image)
        selected = self.sel.make_maps(cc.SELECT_DENSITY)
        uv, typ = self.sel.selection()                                                                # read for the bookkeeping of step 9, and for the host routes
        inside = (uv[:, 0] >= rect[0]) & (uv[:, 0] <= rect[2]) & (uv[:, 1] >= rect[1]) & (uv[:, 1] <= rect[3])
        uv, typ = uv[inside], typ[inside]
        self.seeds[F - 1] = dict(uv=uv, type=typ)
        K = np.asarray(c.K4, np.float64)
        self.before_insert = dict(immature=self.immature_state()) if self.watch else None
        if self.route == "device" and not self.host_flags:
            alive, counts, maps, on_host = _mod("map").seed_immature_from_window(self.imd, F - 1, self.sel, self.w, f.T_w_c, f.T_kf_w, K, c.H, c.W)
            n_map = int(maps["n"][0])
        elif self.route == "device":
            maps = _mod("map").window_depth_maps(self.w, f.T_w_c, [f.T_kf_w], K.reshape(1, 4), c.H, c.W, src_index=False)
            n_map = int(maps["n"][0])
            self.imd.set_depth_map(maps["depth_xy"][0, :n_map], maps["depth_idp"][0, :n_map])
            alive, counts = self.imd.create_points(F - 1, uv, typ)
        else:
            rows = self.ed.rows(state=False)
            ids = self.w_idepths()
            m = mh.window_depth_maps(rows["host"], rows["uv"], ids, np.asarray(c.K4, np.float32), f.T_w_c, (1 << F) - 1, [f.T_kf_w], K.reshape(1, 4), c.H, c.W)[0]
            n_map = len(m["idp"])
            pts, o = dh.seed(self.hl_imd, image, self.imm_prm, dh.tree_of(self.hl_imd, m["xy"], m["idp"]), uv, typ)
            self.pts[F - 1] = pts
            alive = pts["alive"] != 0
            counts = (int(((pts["status"] == no_status("GOOD")) & alive).sum()), int(((pts["status"] == no_status("UNINITIALIZED")) & alive).sum()))
        self.peaks["immature"] = max(self.peaks["immature"], len(uv))
        return dict(selected=np.int32(selected), created=np.int32(len(alive)), alive=np.asarray(alive).astype(np.int32), seeded=np.array(counts, np.int32),
                    map_n=np.int32(n_map))

    def w_idepths(self):
        """the window's idepth_scaled: the solver's row while its state is valid; between marginalize_frame and set_state what was
        read after step 7 (no point leaves or moves in between)"""
        return self.sv.get(system=False)["idepth_scaled"] if self.valid else self.last_ids

    def trace(self, f, cycle):
        c = self.c
        for j in range(2):
            KRKi, Kt, aff = c.trace_inputs(self.ids, cycle, j)
            if self.route == "device":
                if j == 0:
                    self.imm.set_target_images(0, np.stack(c.trace_images[cycle]))
                self.imm.trace(0, [j] * c.F, KRKi, Kt, aff)
            else:
                for h in range(c.F):
                    if len(self.pts[h]):
                        ih.trace(self.hl_imm, self.pts[h], c.trace_images[cycle][j], self.imm_prm, KRKi[h], Kt[h], aff[h])

    def activate(self, f):
        """step 12; returns (points in, residuals in)"""
        c, F = self.c, self.c.F
        rows = self.ed.rows(state=False)
        active = np.concatenate([rows["uv"], self.w_idepths()[:, None]], axis=1).astype(np.float32)
        flagged = np.zeros(F, np.uint8)
        if self.route == "device":
            a = self.act
            a.make_distance_map(F - 1, f.KRKi1, f.Kt1, rows["host"], active)
            a.select(F - 1, f.KRKi1, f.Kt1, flagged, cc.MIN_ACT_DIST)
            a.optimize(f.pre14)
            self.before_insert = self.tables_and_history() if self.watch else None
            ins = np.array(self.ed.insert_activated(a), np.int32)
            self.exchanged(points=True)
            return ins
        hl, w1, h1 = self.hl_act, c.W >> 1, c.H >> 1
        n = np.array([len(p) for p in self.pts], np.int32)
        mp = max(1, int(n.max()))
        pts = np.zeros((F, mp), ih.POINT)
        for h in range(F):
            pts[h, :n[h]] = self.pts[h]
        p_ = ah._p
        K1, T1 = np.ascontiguousarray(f.KRKi1, np.float32), np.ascontiguousarray(f.Kt1, np.float32)
        host = np.ascontiguousarray(rows["host"], np.int32)
        m = np.zeros(w1 * h1, np.uint8)
        hl.act_make_map(w1, h1, F - 1, p_(K1), p_(T1), len(host), p_(host), p_(active), p_(m))
        fate, counts = np.zeros((F, mp), np.int32), np.zeros(10, np.int32)
        pb = ah.pack_params(self.act_prm)
        hl.act_select(p_(pts), mp, p_(n), F - 1, F, p_(K1), p_(T1), p_(flagged), C.c_float(cc.MIN_ACT_DIST), pb, w1, h1, p_(m), p_(fate), p_(counts))
        colors, pre = np.ascontiguousarray(f.images, np.float32), np.ascontiguousarray(f.pre14, np.float32)
        fit, rs, re = np.zeros((F, mp, 4), np.float32), np.zeros((F, mp, F), np.int32), np.zeros((F, mp, F), np.float32)
        fx, fy, cx, cy = (C.c_float(x) for x in c.K4)
        hl.act_optimize(p_(pts), mp, p_(n), F, p_(pre), p_(colors), c.H, c.W, fx, fy, cx, cy, pb, C.c_float(float(self.imm_prm["huber_th"])), p_(fate), p_(fit),
                        p_(rs), p_(re))
        for h in range(F):
            self.pts[h] = pts[h, :n[h]].copy()
        sel = [(h, i) for h in range(F) for i in range(n[h]) if fate[h, i] == ao.ACTIVATED]
        hs, ix = np.array([h for h, _ in sel], np.int32), np.array([i for _, i in sel], np.int32)
        P = pts[hs, ix] if len(sel) else np.zeros(0, ih.POINT)
        activated = dict(host=hs, index=ix, uv=np.stack([P["u"], P["v"]], axis=1).astype(np.float32).reshape(-1, 2), type=P["type"],
                         idepth=(fit[hs, ix, 0] * np.float32(self.act_prm["scale_idepth"])).astype(np.float32) if len(sel) else np.zeros(0, np.float32),
                         color=P["color"].reshape(-1, 8), weights=P["weights"].reshape(-1, 8),
                         target_mask=np.array([sum(1 << t for t in range(F) if rs[h, i, t] == ao.ST_IN) for h, i in sel], np.uint64))
        n_old = self.w.n
        ins = self.ed.insert_activated(activated, F, self.caps[0], self.caps[1])
        self.exchanged(points=True)
        # the history moves by the maps the insert itself formed with edswed::ins_old_point / ins_new_point / ins_old_res / ins_new_res:
        # an old point's columns and an old residual's flag go where their rows went, an activated point has edswfl::activated_point's
        # columns and its residuals are new
        map_p, map_r = self.ed.last_insert_maps()
        new = wfh.activated(None, activated["target_mask"], F)
        src = np.where(map_p >= 0, map_p, n_old + (-2 - map_p))
        hist = {k: np.concatenate([self.hist[k], new[k]])[src] for k in ("num_good", "max_rel_baseline", "last_target", "last_state")}
        hist["is_new"] = np.where(map_r >= 0, self.hist["is_new"][np.maximum(map_r, 0)], 1).astype(np.int32)
        self.hist = hist
        return np.array(ins, np.int32)

    def insert_frame_residuals(self, frame):
        if self.route == "device":
            self.before_insert = self.tables_and_history() if self.watch else None
            K = self.fl.insert_frame_residuals(frame)
        else:
            t = self._arrays()
            _, _, _, self.hist = wfh.insert_frame_residuals(self.hist, t["host"], t["point"], t["target"], frame)
            K = self.ed.insert_frame_residuals(frame, self.caps[1])
        if K:                                                                                          # nothing to insert: nothing is gathered
            self.exchanged(points=False)
        return K

    def refused(self, call):
        """on the device route `call` must be EDS_ERR_STATE: a mark the step before has to have cleared (the host restatements keep no marks)"""
        if self.route != "device":
            return
        capi = _mod("capi")
        try:
            call()
        except capi.EdsError as e:
            assert e.code == capi.ERR_STATE, str(e)
        else:
            raise AssertionError("a call that needs a cleared mark was accepted")

    # ---- the sequence ------------------------------------------------------------------------------------------------------------------------
    def cycle(self, k):
        """cycle k (0-based) on the handles as the last one left them: the list of its snapshots"""
        c, w, sv, ed = self.c, self.w, self.sv, self.ed
        f, F, leaving = self.fi, self.c.F, cc.LEAVING[k]
        snaps = self.snaps = []                                                                        # kept on the driver: a refused call leaves the steps before it there
        snap = lambda step, **out: snaps.append(self.snapshot(k + 1, step, **out))                     # noqa: E731
        parity = np.array([self.exchanges["points"] % 2, self.exchanges["residuals"] % 2], np.int32)
        # 1
        e0, counts = w.linearize(F, f.precalc, f.th)
        w.apply(True)
        sv.fix_linearization((np.arange(w.m) % FIX_EVERY == 3).astype(np.int32))
        snap(1, energy=np.float64(e0), counts=counts, parity=parity)
        # 2
        last, lam, trace, solves = e0, 1e-1, [], []
        for it in range(2):
            sv.backup_idepths()
            sol = sv.solve(it, lam, self.HM, self.bM, MODE, True, None)
            sv.step_idepths(1.0)
            e, counts = w.linearize(F, f.precalc, f.th)
            eL, eM = sv.l_energy(), sv.m_energy(self.HM, self.bM)
            accepted = bool(e + eL + eM < last)
            if accepted:
                w.apply(True)
                last, lam = e + eL + eM, lam * 0.25
            else:
                sv.step_idepths(0.0)
                lam *= 1e2
            # setPrecalcValues -> setDeltaF after the step or its undoing: eds_wed_set_state on a state that is still valid
            ed.set_state(F, f.adH, f.adT, f.delta, f.prior, f.delta_prior, f.cPrior, f.cDelta)
            trace.append(accepted)
            solves.append(dict(x=sol["x"], res_in_a=np.int32(sol["res_in_a"]), res_in_l=np.int32(sol["res_in_l"]), lam=np.float64(sol["lam"]),
                               energy=np.float64(e), l_energy=np.float64(eL), m_energy=np.float64(eM), counts=counts))
        snap(2, accepted=np.array(trace, np.int32), solves=solves)
        # 3
        e, counts = w.linearize(F, f.precalc, f.th)
        states = self.apply_fixed(f)
        snap(3, energy=np.float64(e), counts=counts, states=states)
        # 4
        gone = self.remove_residuals()
        if k % 2 == 1:
            assert tuple(self.remove_no_points()) == (0, 0)
        snap(4, gone=np.int32(gone))
        # 5 .. 7
        fate_counts = self.flag_points(f, 1 << leaving)
        snap(5, fate_counts=fate_counts)
        res_m = self.marginalize_flagged()
        snap(6, res_m=np.int32(res_m), HM=self.HM, bM=self.bM)
        left = self.remove_flagged()
        self.last_ids = sv.get(system=False)["idepth_scaled"]
        self.refused(lambda: self.fl.fates())                                                         # the edit made the fates stale
        snap(7, left=np.array(left, np.int32))
        # 8, 9
        self.marginalize_frame(f, leaving)
        snap(8, HM=self.HM, bM=self.bM)
        self.ids = cc.reindex(self.ids, leaving, c.new_frame[k])
        f = self.fi = c.frame_inputs(self.ids)
        w.set_frames(F - 1, f.images[F - 1])
        self.shift_immature_hosts(leaving, f)
        snap(9, frame=w.frame(F - 1))
        # 10 .. 12
        snap(10, **self.seed_new_keyframe(f))
        self.trace(f, k)
        snap(11)
        inserted = self.activate(f)
        self.refused(lambda: w.apply(True))                                                           # the insert cleared the linearized mark
        snap(12, inserted=inserted)
        # 13
        N = 4 + 8 * F
        HM, bM = np.zeros((N, N)), np.zeros(N)                                                         # the new keyframe's rows and columns: zero
        HM[:N - 8, :N - 8], bM[:N - 8] = self.HM, self.bM
        self.HM, self.bM = HM, bM
        ed.set_state(F, f.adH, f.adT, f.delta, f.prior, f.delta_prior, f.cPrior, f.cDelta)
        self.valid = True
        K = self.insert_frame_residuals(F - 1)
        self.refused(lambda: w.apply(True))                                                           # ... and so did this one
        self.refused(lambda: self.fl.remove_flagged())                                                # no fates are current
        snap(13, inserted=np.int32(K))
        return snaps


def no_status(name):
    return no.STATUS_NAMES.index(name)


def run(route, case=None, cycles=cc.CYCLES, **kw):
    """the snapshots of `cycles` cycles on fresh handles of `route`, one after every numbered step of every cycle, and the driver's peaks"""
    d = Driver(route, case, **kw)
    try:
        snaps = [s for k in range(cycles) for s in d.cycle(k)]
        return snaps, dict(d.peaks)
    finally:
        d.close()


def first_difference(a, b):
    """the first (cycle, step, key) at which two runs' snapshots differ bit for bit (any NaN equal to any NaN), or None"""
    for x, y in zip(a, b):
        fx, fy = dict(wsh.flatten(x)), dict(wsh.flatten(y))
        for key in fx:
            if key not in fy or not wsh.same_bits(fx[key], fy[key]):
                return x["cycle"], x["step"], key
        if set(fy) - set(fx):
            return x["cycle"], x["step"], sorted(set(fy) - set(fx))[0]
    return None if len(a) == len(b) else ("length", len(a), len(b))
