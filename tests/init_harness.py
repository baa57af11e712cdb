"""ctypes side of tests/host_logic/init_harness.cpp: csrc/eds_init.hpp (namespace edsini, what the device kernels run) compiled with g++
into a temporary directory where the tests run — ``HostInitializer`` has the methods of ``slam-eds_amd.init.CoarseInitializer`` plus the
single steps the oracle tests compare — and the stand-alone program of the same source."""
import ctypes as C
import os
import subprocess

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "init_harness.cpp")

# edsini::Pnt / eds_ini_point, edsini::Result / eds_ini_result, edsini::Sys
POINT = np.dtype([("u", "f4"), ("v", "f4"), ("idepth", "f4"), ("idepth_new", "f4"), ("iR", "f4"), ("lastHessian", "f4"), ("lastHessian_new", "f4"),
                  ("maxstep", "f4"), ("energy", "f4", 2), ("energy_new", "f4", 2), ("my_type", "f4"), ("outlierTH", "f4"), ("isGood", "i4"),
                  ("isGood_new", "i4")])
RESULT = np.dtype([("T", "f8", (3, 4)), ("aff", "f8", 2), ("latest_res", "f4", 3), ("rescale", "f4"), ("snapped", "i4"), ("frame_id", "i4"),
                   ("snapped_at", "i4"), ("ready", "i4"), ("n_decisions", "i4"), ("launches", "i4"), ("waits", "i4"), ("reserved", "i4"),
                   ("iterations", "i4", 5), ("accepts", "i4", 5), ("decisions", "u1", 512)])
SYS = np.dtype([("H", "f4", (8, 8)), ("b", "f4", 8), ("Hsc", "f4", (8, 8)), ("bsc", "f4", 8), ("res", "f4", 3), ("pad", "f4")])
PARAMS = np.dtype([("huber_th", "f4"), ("outlier_th", "f4"), ("alpha_k", "f4"), ("alpha_w", "f4"), ("reg_weight", "f4"), ("coupling_weight", "f4"),
                   ("fix_affine", "i4"), ("max_iterations", "i4", 5), ("scale_xi_rot", "f4"), ("scale_xi_trans", "f4"), ("scale_a", "f4"),
                   ("scale_b", "f4")])
CARRY = np.dtype([("T", "f8", (3, 4)), ("aff", "f8", 2), ("snapped", "i4"), ("frame_id", "i4"), ("snapped_at", "i4"), ("jb_cur", "i4", 5)])

_lib = None
_vp = hb.p


def load_harness():
    global _lib
    if _lib is None:
        L = hb.load_library("init", SRC)
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        assert L.ini_sizes(C.byref(a), C.byref(b), C.byref(c)) == 512
        assert (a.value, b.value, c.value) == (POINT.itemsize, RESULT.itemsize, SYS.itemsize) == (64, 712, 592)
        vp, f, i = C.c_void_p, C.c_float, C.c_int
        L.ini_create.restype = vp
        for name, args in dict(ini_create=[i] * 4, ini_destroy=[vp], ini_set_params=[vp, vp], ini_set_calib=[vp, f, f, f, f], ini_set_first=[vp, vp, f],
                               ini_set_pose=[vp, vp, vp], ini_set_points=[vp, i, vp], ini_make_nn=[i, vp, i, vp, vp, vp],
                               ini_set_neighbours=[vp, i, vp, vp], ini_schedule_depth=[vp, i], ini_track_frame=[vp, vp, f, i, vp],
                               ini_get_points=[vp, i, vp], ini_set_points_state=[vp, i, vp], ini_get_jb=[vp, i, i, vp], ini_set_jb=[vp, i, i, vp],
                               ini_get_level=[vp, i, i, vp], ini_set_new=[vp, vp], ini_get_carry=[vp, vp], ini_first_loop=[vp, i, vp, vp, vp, vp, vp],
                               ini_calc=[vp, i, vp, vp, vp, vp], ini_calc_ec=[vp, i, i, vp], ini_do_step=[vp, i, f, vp], ini_apply_step=[vp, i],
                               ini_opt_reg=[vp, i, i], ini_reset_points=[vp, i], ini_propagate_down=[vp, i, i], ini_propagate_up=[vp, i, i],
                               ini_solve_inc=[vp, vp, f, i, vp], ini_atan_n=[vp, i, vp], ini_log_upsilon=[vp, vp], ini_params_default=[vp]).items():
            getattr(L, name).argtypes = args
        _lib = L
    return _lib


def default_params(**over):
    p = np.zeros(1, PARAMS)
    load_harness().ini_params_default(_vp(p))
    for k, v in over.items():
        p[k] = v
    return p


def atan(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    load_harness().ini_atan_n(_vp(x), x.size, _vp(out))
    return out


def log_upsilon(T):
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(12)
    out = np.zeros(3)
    load_harness().ini_log_upsilon(_vp(T), _vp(out))
    return out


def make_nn(uv, uv_up=None):
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    nb = np.full((len(uv), 10), -1, np.int32)
    if uv_up is None:
        load_harness().ini_make_nn(len(uv), _vp(uv), 0, None, _vp(nb), None)
        return nb, None
    up = np.ascontiguousarray(uv_up, dtype=np.float32).reshape(-1, 2)
    parent = np.zeros(len(uv), np.int32)
    load_harness().ini_make_nn(len(uv), _vp(uv), len(up), _vp(up), _vp(nb), _vp(parent))
    return nb, parent


class HostInitializer:
    """edsini:: under g++ behind the interface of slam-eds_amd.init.CoarseInitializer"""

    def __init__(self, H, W, levels=5, max_points_per_level=16384, **params):
        self.L = load_harness()
        self.H, self.W, self.levels, self.cap = H, W, levels, max_points_per_level
        self._h = self.L.ini_create(H, W, levels, max_points_per_level)
        assert self._h, "shape refused"
        self.prm = default_params()
        self.n = np.zeros(levels, np.int32)
        self.last = None
        if params:
            self.set_params(**params)

    def close(self):
        if self._h:
            self.L.ini_destroy(self._h)
            self._h = None

    def set_params(self, **over):
        for k, v in over.items():
            self.prm[k] = v
        assert self.L.ini_set_params(self._h, _vp(self.prm)) == 0

    def set_calib(self, fx, fy, cx, cy):
        self.L.ini_set_calib(self._h, fx, fy, cx, cy)

    def setFirst(self, image, exposure=1.0):
        self.L.ini_set_first(self._h, _vp(np.ascontiguousarray(image, dtype=np.float32)), exposure)

    def set_pose(self, T, aff=(0.0, 0.0)):
        self.L.ini_set_pose(self._h, _vp(np.ascontiguousarray(T, dtype=np.float64).reshape(12)), _vp(np.ascontiguousarray(aff, dtype=np.float64)))

    def set_points(self, lvl, status):
        n = self.L.ini_set_points(self._h, lvl, _vp(np.ascontiguousarray(status, dtype=np.float32)))
        assert n <= self.cap
        self.n[lvl] = n
        return n

    def set_neighbours(self, lvl, nb, parent=None):
        nb = np.ascontiguousarray(nb, dtype=np.int32)
        par = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
        assert self.L.ini_set_neighbours(self._h, lvl, _vp(nb), _vp(par)) == 0

    def schedule_depth(self, lvl):
        return self.L.ini_schedule_depth(self._h, lvl)

    def trackFrame(self, image, exposure=1.0, snapped_threshold=5):
        out = np.zeros(1, RESULT)
        self.L.ini_track_frame(self._h, _vp(np.ascontiguousarray(image, dtype=np.float32)), exposure, snapped_threshold, _vp(out))
        self.last = out[0]
        return out[0]

    def rescale(self):
        return float(self.last["rescale"])

    def points(self, lvl):
        out = np.zeros(int(self.n[lvl]), POINT)
        self.L.ini_get_points(self._h, lvl, _vp(out))
        return out

    def jb(self, lvl, which):
        out = np.zeros((int(self.n[lvl]), 10), np.float32)
        self.L.ini_get_jb(self._h, lvl, which, _vp(out))
        return out

    def level(self, which, lvl):
        out = np.zeros((self.H >> lvl, self.W >> lvl, 3), np.float32)
        self.L.ini_get_level(self._h, which, lvl, _vp(out))
        return out

    # ---- what only the host restatement has: its state set from outside, and the single steps --------------------------------------------
    def carry(self):
        out = np.zeros(1, CARRY)
        self.L.ini_get_carry(self._h, _vp(out))
        return out[0]

    def set_new(self, image):
        self.L.ini_set_new(self._h, _vp(np.ascontiguousarray(image, dtype=np.float32)))

    def set_state(self, lvl, pts, jb=None):
        self.L.ini_set_points_state(self._h, lvl, _vp(np.ascontiguousarray(pts)))
        if jb is not None:
            self.L.ini_set_jb(self._h, lvl, 0, _vp(np.ascontiguousarray(jb, dtype=np.float32)))

    def first_loop(self, lvl, T, aff):
        n = int(self.n[lvl])
        rows, taps, sums = np.zeros((n, 10), np.float32), np.full((n, 8, 2), np.nan, np.float32), np.zeros(46)
        self.L.ini_first_loop(self._h, lvl, _vp(np.ascontiguousarray(T, dtype=np.float64).reshape(12)), _vp(np.ascontiguousarray(aff, dtype=np.float64)),
                              _vp(rows), _vp(taps), _vp(sums))
        return rows, taps, sums

    def calc(self, lvl, T, aff):
        out, self.sc_sums = np.zeros(1, SYS), np.zeros(45)
        self.L.ini_calc(self._h, lvl, _vp(np.ascontiguousarray(T, dtype=np.float64).reshape(12)), _vp(np.ascontiguousarray(aff, dtype=np.float64)), _vp(out),
                        _vp(self.sc_sums))
        return out[0]

    def calc_ec(self, lvl, snapped):
        out = np.zeros(3, np.float32)
        self.L.ini_calc_ec(self._h, lvl, int(snapped), _vp(out))
        return out

    def do_step(self, lvl, lam, inc):
        self.L.ini_do_step(self._h, lvl, lam, _vp(np.ascontiguousarray(inc, dtype=np.float32)))

    def apply_step(self, lvl):
        self.L.ini_apply_step(self._h, lvl)

    def opt_reg(self, lvl, snapped):
        self.L.ini_opt_reg(self._h, lvl, int(snapped))

    def reset_points(self, lvl):
        self.L.ini_reset_points(self._h, lvl)

    def propagate_down(self, src, snapped):
        self.L.ini_propagate_down(self._h, src, int(snapped))

    def propagate_up(self, src, snapped):
        self.L.ini_propagate_up(self._h, src, int(snapped))


def solve_inc(sys_rec, prm, lam, wh):
    inc = np.zeros(8, np.float32)
    s = np.zeros(1, SYS)
    s[0] = sys_rec
    load_harness().ini_solve_inc(_vp(s), _vp(prm), lam, wh, _vp(inc))
    return inc


def open_case(c, cls=HostInitializer, **kw):
    """an initialiser of class `cls` holding case c's calibration, parameters, first frame, points and tables"""
    t = cls(c.H, c.W, c.levels, max_points_per_level=c.cap, **kw)
    t.set_params(**c.prm)
    t.set_calib(*c.K)
    t.setFirst(c.first, c.exposures[0])
    for l in range(c.levels):
        assert t.set_points(l, c.status[l]) == len(c.uv[l])
    for l in range(c.levels):
        t.set_neighbours(l, c.nb[l], c.parent[l])
    if c.pose_guess is not None:
        t.set_pose(c.pose_guess)
    return t


def run_standalone(extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all) and runs it once"""
    exe, _ = hb.build_program("init", SRC, "INI_STANDALONE", extra_flags)
    return subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/init_harness.py [g++ flags]: the sanitizer run of DESIGN §24
    import sys
    print(run_standalone(sys.argv[1:]), end="")
