"""ctypes side of tests/host_logic/winedit_harness.cpp: csrc/eds_winedit.hpp (namespace edswed, what the device kernels run) compiled
with g++ into the temporary directory of tests/window_harness.py — ``HostEdit`` has the methods of ``slam-eds_amd.winedit.WindowEdit``
over a ``winsolve_harness.HostWindow`` / ``HostSolver`` —, the sequence both sides run before an edit, the snapshot of every row a
caller can read, and the stand-alone program of the same source."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb
import window_harness as wh
import winsolve_harness as wsh

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "winedit_harness.cpp")
OUT_FIELDS = (("point", "i4", lambda m, n: (m,)), ("target", "i4", lambda m, n: (m,)), ("res_first", "i4", lambda m, n: (n + 1,)),
              ("host", "i4", lambda m, n: (n,)), ("uv", "f4", lambda m, n: (n, 2)), ("color", "f4", lambda m, n: (n, 8)),
              ("weights", "f4", lambda m, n: (n, 8)), ("idepth_zero_scaled", "f4", lambda m, n: (n,)), ("deltaF", "f4", lambda m, n: (n,)),
              ("idepth_backup", "f4", lambda m, n: (n,)))
STATE_FIELDS = ("idepth_backup",)
# what eds_wsv_get returns per residual and per point (the frame-sized results of a solve are not rows)
WSV_ROWS = ("is_linearized", "res_toZeroF", "resApprox", "lf", "step", "idepth_scaled", "priorF")

_lib = None
_vp = hb.p


def load_harness():
    """the wed_* functions; they work on the objects winsolve_harness.load_harness() creates (one source, one layout)"""
    global _lib
    if _lib is None:
        wsh.load_harness()
        L = hb.load_library("winedit", SRC)
        vp = C.c_void_p
        L.wed_remove_residuals.argtypes = [vp, vp, vp, vp]
        L.wed_remove_points.argtypes = [vp, vp, vp, vp, vp]
        L.wed_marg_arith.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        L.wed_inverse8.argtypes = [vp, vp]
        L.wed_marginalize_frame.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.wed_set_state.argtypes = [vp, vp, C.c_int] + [vp] * 7
        L.wed_insert_activated.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int, C.c_int, vp, vp]
        L.wed_insert_frame_residuals.argtypes = [vp, vp, C.c_int, C.c_int, vp]
        L.wed_reset_oob.argtypes = [vp, vp, vp]
        L.wed_last_insert_maps.argtypes = [C.c_int, C.c_int, vp, vp]
        L.wed_forget.argtypes = [vp]
        L.wed_counts.argtypes = [vp, vp, vp, vp]
        L.wed_edit_mirrors.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        L.wed_get.argtypes = [vp, vp, vp]
        _lib = L
    return _lib


def _i32(a, count):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(count)


class HostEdit:
    """edswed:: under g++ behind the interface of slam-eds_amd.winedit.WindowEdit"""

    def __init__(self, win, solver=None):
        self.L = load_harness()
        self.win = win
        if self._s():
            self.L.wed_forget(self._s())                         # a new solver may sit where a closed one sat

    def _s(self):
        return self.win.solver._s if getattr(self.win, "solver", None) else None

    def marginalize_frame(self, frame, prior, delta_prior, HM, bM):
        bm = wsh._f64(bM, (-1,))
        N = len(bm)
        out_h, out_b = np.zeros((max(N - 8, 0), max(N - 8, 0))), np.zeros(max(N - 8, 0))
        wsh._rc(self.L.wed_marginalize_frame(self.win._h, self._s(), int(frame), _vp(wsh._f64(prior, (8,))), _vp(wsh._f64(delta_prior, (8,))),
                                             _vp(wsh._f64(HM, (N, N))), _vp(bm), _vp(out_h), _vp(out_b)))
        self.win.n, self.win.m, _ = self.counts()
        return out_h, out_b

    def set_state(self, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta):
        f = wsh._f64
        wsh._rc(self.L.wed_set_state(self.win._h, self._s(), F, _vp(f(adHost, (F * F, 8, 8))), _vp(f(adTarget, (F * F, 8, 8))), _vp(f(delta, (F, 8))),
                                     _vp(f(prior, (F, 8))), _vp(f(delta_prior, (F, 8))), _vp(f(cPrior, (4,))), _vp(f(cDelta, (4,)))))
        self.win.solver.F = F

    def insert_activated(self, activated, F, max_points=1 << 22, max_residuals=1 << 24):
        """`activated`: what Activation.activated() returns (the device entry point reads the same values from the eds_imm)"""
        a = activated
        K = len(a["host"])
        mp = int(a["index"].max()) + 1 if K else 1
        f32 = lambda x, sh: np.ascontiguousarray(x, dtype=np.float32).reshape(sh)      # noqa: E731
        ip, ir = C.c_int32(), C.c_int32()
        wsh._rc(self.L.wed_insert_activated(self.win._h, self._s(), int(F), mp, K, _vp(_i32(a["host"], K)), _vp(_i32(a["index"], K)), _vp(f32(a["uv"], (K, 2))),
                                            _vp(f32(a["color"], (K, 8))), _vp(f32(a["weights"], (K, 8))), _vp(f32(a["idepth"], (K,))),
                                            _vp(np.ascontiguousarray(a["target_mask"], dtype=np.uint64).reshape(K)), int(max_points), int(max_residuals),
                                            C.cast(C.byref(ip), C.c_void_p), C.cast(C.byref(ir), C.c_void_p)))
        self.win.n += ip.value
        self.win.m += ir.value
        self.linearized = False
        return ip.value, ir.value

    def last_insert_maps(self):
        """where the last ``insert_activated`` put the rows: (new point row -> old row, or -2 - k for the k-th activated point; new
        residual row -> old row, or -1 for a new residual)"""
        map_p, map_r = np.zeros(self.win.n, np.int32), np.zeros(self.win.m, np.int32)
        wsh._rc(self.L.wed_last_insert_maps(self.win.n, self.win.m, _vp(map_p), _vp(map_r)))
        return map_p, map_r

    def insert_frame_residuals(self, frame, max_residuals=1 << 24):
        """the rows' half of ``WindowFlags.insert_frame_residuals`` (the history's is ``winflag_harness.insert_frame_residuals``)"""
        inserted = C.c_int32()
        wsh._rc(self.L.wed_insert_frame_residuals(self.win._h, self._s(), int(frame), int(max_residuals), C.cast(C.byref(inserted), C.c_void_p)))
        self.win.m += inserted.value
        return inserted.value

    def reset_oob(self, mask):
        """``resetOOB`` and isLinearized = 0 for every residual of the points with mask != 0: the first step of the re-linearization in
        ``WindowFlags.flag_points``"""
        wsh._rc(self.L.wed_reset_oob(self.win._h, self._s(), _vp(_i32(mask, self.win.n))))

    def remove_residuals(self, select=None):
        sel = None if select is None else _i32(select, self.win.m)
        removed = C.c_int32()
        wsh._rc(self.L.wed_remove_residuals(self.win._h, self._s(), _vp(sel), C.cast(C.byref(removed), C.c_void_p)))
        self.win.m -= removed.value
        return removed.value

    def remove_points(self, flag):
        rp, rr = C.c_int32(), C.c_int32()
        wsh._rc(self.L.wed_remove_points(self.win._h, self._s(), _vp(_i32(flag, self.win.n)), C.cast(C.byref(rp), C.c_void_p), C.cast(C.byref(rr), C.c_void_p)))
        self.win.n -= rp.value
        self.win.m -= rr.value
        return rp.value, rr.value

    def counts(self):
        n, m, per_host = C.c_int32(), C.c_int32(), np.zeros(8, np.int32)
        wsh._rc(self.L.wed_counts(self.win._h, C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(m), C.c_void_p), _vp(per_host)))
        return n.value, m.value, per_host

    def rows(self, state=True):
        m, n = self.win.m, self.win.n
        out = {k: np.zeros(sh(m, n), dt) for k, dt, sh in OUT_FIELDS}
        ptrs = [out[k].ctypes.data if (state or k not in STATE_FIELDS) else 0 for k, _, _ in OUT_FIELDS]
        wsh._rc(self.L.wed_get(self.win._h, self._s(), struct.pack(f"<{len(ptrs)}Q", *ptrs)))
        return {k: v for k, v in out.items() if state or k not in STATE_FIELDS}


def marg_arith(frame, prior, delta_prior, HM, bM):
    """edswed::marg_frame_body by one thread: (rc, HM', bM')"""
    bm = wsh._f64(bM, (-1,))
    N = len(bm)
    out_h, out_b = np.zeros((N - 8, N - 8)), np.zeros(N - 8)
    rc = load_harness().wed_marg_arith(N, int(frame), _vp(wsh._f64(HM, (N, N))), _vp(bm), _vp(wsh._f64(prior, (8,))), _vp(wsh._f64(delta_prior, (8,))),
                                       _vp(out_h), _vp(out_b))
    return rc, out_h, out_b


def inverse8(a):
    """the stated 8 x 8 inverse: (rc, hpi)"""
    out = np.zeros((8, 8))
    rc = load_harness().wed_inverse8(_vp(wsh._f64(a, (8, 8))), _vp(out))
    return rc, out


def edit_mirrors(host_of, point, target, keep_p, keep_r):
    """edswed::edit_mirrors: (host_of, point, target, max_host, max_target) of the window's host copies after an edit"""
    n, m = len(host_of), len(point)
    h, p, t = _i32(host_of, n).copy(), _i32(point, m).copy(), _i32(target, m).copy()
    out = np.zeros(4, np.int32)
    kp = None if keep_p is None else _i32(keep_p, n)
    load_harness().wed_edit_mirrors(n, m, _vp(h), _vp(p), _vp(t), _vp(kp), _vp(_i32(keep_r, m)), _vp(out))
    return h[:out[0]], p[:out[1]], t[:out[1]], int(out[2]), int(out[3])


def prepare(w, sv, s):
    """the calls before an edit: linearize -> apply -> set_state -> fix_linearization -> backup -> solve -> step"""
    c = s.win
    wsh.lin_apply(w, s)
    sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
    sv.fix_linearization(s.fix)
    sv.backup_idepths()
    r = s.rounds[0]
    sv.solve(r.iteration, r.lam, s.HM, s.bM, r.mode, r.hff, s.P if r.use_p else None)
    sv.step_idepths(r.fac)


def snapshot(w, sv, ed):
    """every row a caller can read: eds_win_get_residuals, eds_win_get_points, the rows of eds_wsv_get, eds_wed_get, and the counts"""
    n, m, per_host = ed.counts()
    assert (n, m) == (w.n, w.m)
    state = sv.get(system=False)
    return dict(residuals=w.residuals(), points=w.points(), state={k: state[k] for k in WSV_ROWS}, rows=ed.rows(),
                counts=np.array([n, m], np.int32), per_host=per_host)


def run_pattern(w, sv, ed, s, pattern, steps_of):
    """prepare, for "marginalised" the point marginalisation, then the pattern's steps (steps_of: winedit_cases.steps): the snapshots
    before the first step and after every step (with what the step reports as removed), and the marginalised (HM, bM) or the case's"""
    prepare(w, sv, s)
    HM, bM = s.HM, s.bM
    if pattern == "marginalised":
        sv.fix_linearization(s.fix_marg)
        HM, bM, _ = sv.marginalize_points(s.marg, s.HM, s.bM, prior_fac=wsh.PRIOR_FAC, weight_fac=wsh.WEIGHT_FAC)
    snaps = [snapshot(w, sv, ed)]
    rows = snaps[0]["rows"]
    for kind, flags in steps_of(pattern, s, w.n, w.m, rows["host"], rows["point"]):
        removed = ed.remove_points(flags) if kind == "points" else ed.remove_residuals(flags)
        snaps.append(snapshot(w, sv, ed))
        snaps[-1]["removed"] = np.atleast_1d(np.array(removed, np.int32))
    return snaps, HM, bM


def run_frame(w, sv, ed, s, frame, reduce_case):
    """prepare, the points the frame hosts removed (a hosted point is refused), eds_wed_marginalize_frame with the case's HM, bM and the
    frame's priors, eds_wed_set_state for the F - 1 frames left, and what the window does next: everything read back"""
    prepare(w, sv, s)
    F = s.F
    ed.remove_points((ed.rows()["host"] == frame).astype(np.int32))
    before = snapshot(w, sv, ed)
    frames_before = np.stack([w.frame(f) for f in range(F)])
    HM, bM = ed.marginalize_frame(frame, s.prior[frame], s.delta_prior[frame], s.HM, s.bM)
    r = reduce_case(s, frame)
    ed.set_state(r.F, r.win.adH, r.win.adT, r.delta, r.prior, r.delta_prior, r.cPrior, r.cDelta)
    after = snapshot(w, sv, ed)
    frames = np.stack([w.frame(f) for f in range(r.F)])
    nxt = after_edit(w, sv, r, HM, bM, full=True, accumulate=False)
    return dict(before=before, frames_before=frames_before, after=after, HM=HM, bM=bM, frames=frames, next=nxt)


def after_edit(w, sv, s, HM, bM, full=True, accumulate=True):
    """the window goes on after an edit: linearize -> apply, and with `full` eds_win_accumulate and a solve with the point steps:
    everything read back.  An OOB residual's J is whatever it was before (nothing reads it): zeroed here."""
    c = s.win
    energy, counts = w.linearize(c.F, c.precalc, c.th)
    lin = w.residuals()
    w.apply(True)
    res = w.residuals()
    out = dict(energy=np.float64(energy), counts=counts, new_state=lin["new_state"], new_energy=lin["new_energy"], state=res["state"],
               res_energy=res["energy"], is_active=res["is_active"])
    J = lin["J"].copy()
    J[lin["new_state"] == 1] = 0
    out["J"] = J
    if full and accumulate:                                      # the host window's accumulate knows no linearized flag: only without them
        out["accumulated"] = w.accumulate(c.F, c.adH, c.adT, None, None, None, False)
    if full:
        r = s.rounds[0]
        out["solve"] = sv.solve(r.iteration, r.lam, HM, bM, r.mode, r.hff, s.P if r.use_p else None)
        out["steps"] = sv.steps()
        out["points"] = w.points()
    return out


def run_standalone(cases, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -g -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` (winsolve cases) plus its own hostile flags, returns its output; raises when it fails"""
    exe, data = hb.build_program("winedit", SRC, "WED_STANDALONE", extra_flags)
    wsh.dump_cases(data, cases)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/winedit_harness.py [g++ flags]: the sanitizer run of DESIGN §21
    import sys
    sys.path.insert(0, HERE)
    import winsolve_cases as wsc
    print(run_standalone(list(wsc.cases().values()), sys.argv[1:]), end="")
