"""ctypes side of tests/host_logic/window_harness.cpp: csrc/eds_window.hpp (namespace edswin, what the device kernels run) compiled with
g++ into a temporary directory where the tests run — ``HostWindow`` has the methods of ``slam-eds_amd.window.Window`` — and the
stand-alone program of the same source with the cases dumped for it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_logic", "window_harness.cpp")
PARAM_ORDER = ("outlier_th_sum_component", "huber_th", "affine_opt_mode_a", "affine_opt_mode_b", "scale_idepth", "scale_f", "scale_c")
DEFAULTS = dict(outlier_th_sum_component=2500.0, huber_th=9.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8, scale_idepth=1.0, scale_f=1.0,
                scale_c=1.0)
J_WORDS = 74
RESIDUAL_FIELDS = (("state", "i4", ()), ("energy", "f4", ()), ("new_state", "i4", ()), ("new_energy", "f4", ()),
                   ("new_energy_with_outlier", "f4", ()), ("linearize_return", "f4", ()), ("is_active", "i4", ()),
                   ("center_projected_to", "f4", (3,)), ("projected_to", "f4", (8, 2)), ("J", "f4", (J_WORDS,)), ("ef_J", "f4", (J_WORDS,)),
                   ("JpJdF", "f4", (8,)))
POINT_FIELDS = (("Hdd_accAF", "f4", ()), ("bd_accAF", "f4", ()), ("Hcd_accAF", "f4", (4,)), ("HdiF", "f4", ()), ("bdSumF", "f4", ()),
                ("idepth_hessian", "f4", ()), ("nres", "i4", ()))


def pack_params(prm):
    return b"".join(struct.pack("<f", prm[k]) for k in PARAM_ORDER) + struct.pack("<f", 0.0)


_lib = None


def load_harness():
    global _lib
    if _lib is None:
        L = hb.load_library("window", SRC)
        a, b = C.c_int(), C.c_int()
        assert L.win_sizes(C.byref(a), C.byref(b)) == 76 and a.value == J_WORDS and b.value == 512
        vp, f = C.c_void_p, C.c_float
        L.win_create.restype = vp
        L.win_create.argtypes = [C.c_int] * 3
        L.win_destroy.argtypes = [vp]
        L.win_set_params.argtypes = [vp, vp]
        L.win_set_calib.argtypes = [vp, f, f, f, f]
        L.win_set_frames.argtypes = [vp, C.c_int, C.c_int, vp]
        L.win_get_frame.argtypes = [vp, C.c_int, vp]
        L.win_set_points.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.win_set_idepths.argtypes = [vp, vp, vp]
        L.win_set_residuals.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.win_linearize.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.win_apply.argtypes = [vp, C.c_int]
        L.win_point_hessians.argtypes = [vp, vp, vp, vp, C.c_int]
        L.win_get_residuals.argtypes = [vp, vp]
        L.win_accumulate.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        L.win_get_points.argtypes = [vp, vp]
        L.win_stitch_entries.argtypes = [C.c_int, vp, vp, vp, vp]
        L.win_linearize_points.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]
        L.win_linearize_fold.argtypes = [vp, vp]
        L.win_linearize_fold.restype = C.c_double
        L.win_apply_points.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.win_point_hessians_points.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int]
        _lib = L
    return _lib


_vp = hb.p


def _f32(a, shape):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(shape)


class HostWindow:
    """edswin:: under g++ behind the interface of slam-eds_amd.window.Window"""

    def __init__(self, H, W, max_frames=8, **params):
        self.L = load_harness()
        self.H, self.W, self.max_frames = H, W, max_frames
        self._h = self.L.win_create(H, W, max_frames)
        assert self._h, "shape refused"
        self.prm = dict(DEFAULTS)
        self.n = self.m = 0
        if params:
            self.set_params(**params)

    def close(self):
        if self._h:
            self.L.win_destroy(self._h)
            self._h = None

    def set_params(self, **over):
        self.prm.update(over)
        assert self.L.win_set_params(self._h, pack_params(self.prm)) == 0

    def set_calib(self, fx, fy, cx, cy):
        self.L.win_set_calib(self._h, fx, fy, cx, cy)

    def set_frames(self, first, images):
        a = np.ascontiguousarray(images, dtype=np.float32)
        a = a[None] if a.ndim == 2 else a
        self.L.win_set_frames(self._h, first, len(a), _vp(a))

    def frame(self, f):
        out = np.zeros((self.H, self.W, 3), np.float32)
        self.L.win_get_frame(self._h, f, _vp(out))
        return out

    def set_points(self, host, uv, color, weights, idepth_scaled, idepth_zero_scaled=None):
        host = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
        n = len(host)
        ids = _f32(idepth_scaled, (n,))
        idz = ids if idepth_zero_scaled is None else _f32(idepth_zero_scaled, (n,))
        assert self.L.win_set_points(self._h, n, _vp(host), _vp(_f32(uv, (n, 2))), _vp(_f32(color, (n, 8))), _vp(_f32(weights, (n, 8))), _vp(ids), _vp(idz)) == 0
        self.n, self.m = n, 0

    def set_idepths(self, idepth_scaled=None, idepth_zero_scaled=None):
        ids = None if idepth_scaled is None else _f32(idepth_scaled, (self.n,))
        idz = None if idepth_zero_scaled is None else _f32(idepth_zero_scaled, (self.n,))
        self.L.win_set_idepths(self._h, _vp(ids), _vp(idz))

    def set_residuals(self, point, target, state=None, energy=None):
        point = np.ascontiguousarray(point, dtype=np.int32).reshape(-1)
        m = len(point)
        target = np.ascontiguousarray(target, dtype=np.int32).reshape(m)
        st = None if state is None else np.ascontiguousarray(state, dtype=np.int32).reshape(m)
        en = None if energy is None else _f32(energy, (m,))
        assert self.L.win_set_residuals(self._h, m, _vp(point), _vp(target), _vp(st), _vp(en)) == 0
        self.m = m

    def linearize(self, F, precalc, frame_energy_th):
        e, counts = C.c_double(), np.zeros(3, np.int32)
        assert self.L.win_linearize(self._h, F, _vp(_f32(precalc, (F * F, 27))), _vp(_f32(frame_energy_th, (F,))), C.cast(C.byref(e), C.c_void_p), _vp(counts)) == 0
        return e.value, counts

    def apply(self, copy_jacobians=True):
        self.L.win_apply(self._h, 1 if copy_jacobians else 0)

    def point_hessians(self, priorF=None, deltaF=None, lf=None, shift_prior_to_zero=False):
        pr = None if priorF is None else _f32(priorF, (self.n,))
        de = None if deltaF is None else _f32(deltaF, (self.n,))
        l = None if lf is None else _f32(lf, (self.n, 6))
        return self.L.win_point_hessians(self._h, _vp(pr), _vp(de), _vp(l), 1 if shift_prior_to_zero else 0)

    # the same three stages with the points sliced by `grain` over a pool of threads (ctypes releases the GIL during a call); the
    # energy is folded afterwards in the header's order, so every result equals the one-thread call's bit for bit
    def _slices(self, grain):
        return [(p, min(p + grain, self.n)) for p in range(0, self.n, grain)]

    def linearize_pool(self, pool, F, precalc, frame_energy_th, grain=50):
        pc, th = _f32(precalc, (F * F, 27)), _f32(frame_energy_th, (F,))
        list(pool.map(lambda s: self.L.win_linearize_points(self._h, F, _vp(pc), _vp(th), s[0], s[1]), self._slices(grain)))
        counts = np.zeros(3, np.int32)
        return self.L.win_linearize_fold(self._h, _vp(counts)), counts

    def apply_pool(self, pool, copy_jacobians=True, grain=50):
        list(pool.map(lambda s: self.L.win_apply_points(self._h, 1 if copy_jacobians else 0, s[0], s[1]), self._slices(grain)))

    def point_hessians_pool(self, pool, priorF, deltaF, lf, shift_prior_to_zero=False, grain=50):
        pr, de, l = _f32(priorF, (self.n,)), _f32(deltaF, (self.n,)), _f32(lf, (self.n, 6))
        return sum(pool.map(lambda s: self.L.win_point_hessians_points(self._h, _vp(pr), _vp(de), _vp(l), 1 if shift_prior_to_zero else 0, s[0], s[1]),
                            self._slices(grain)))

    def accumulate(self, F, adHost, adTarget, priorF=None, deltaF=None, lf=None, shift_prior_to_zero=False):
        """dict(H_A, b_A, H_sc, b_sc, acc, nres)"""
        N = 4 + 8 * F
        adH, adT = (np.ascontiguousarray(a, dtype=np.float64).reshape(F * F, 8, 8) for a in (adHost, adTarget))
        pr = None if priorF is None else _f32(priorF, (self.n,))
        de = None if deltaF is None else _f32(deltaF, (self.n,))
        l = None if lf is None else _f32(lf, (self.n, 6))
        out = dict(H_A=np.zeros((N, N)), b_A=np.zeros(N), H_sc=np.zeros((N, N)), b_sc=np.zeros(N), acc=np.zeros(self.L.win_acc_size(F)))
        nres = self.L.win_accumulate(self._h, F, _vp(adH), _vp(adT), _vp(pr), _vp(de), _vp(l), 1 if shift_prior_to_zero else 0, _vp(out["H_A"]),
                                     _vp(out["b_A"]), _vp(out["H_sc"]), _vp(out["b_sc"]), _vp(out["acc"]))
        assert nres >= 0, "refused"
        out["nres"] = np.int32(nres)
        return out

    def residuals(self):
        out = {k: np.zeros((self.m,) + sh, dt) for k, dt, sh in RESIDUAL_FIELDS}
        self.L.win_get_residuals(self._h, struct.pack("<12Q", *(out[k].ctypes.data for k, _, _ in RESIDUAL_FIELDS)))
        return out

    def points(self):
        out = {k: np.zeros((self.n,) + sh, dt) for k, dt, sh in POINT_FIELDS}
        self.L.win_get_points(self._h, struct.pack("<7Q", *(out[k].ctypes.data for k, _, _ in POINT_FIELDS)))
        return out


def stitch_entries(F, acc, adHost, adTarget):
    """both stitches entry by entry: (H_A, b_A, H_sc, b_sc)"""
    N = 4 + 8 * F
    adH, adT = (np.ascontiguousarray(a, dtype=np.float64).reshape(F * F, 8, 8) for a in (adHost, adTarget))
    out = np.zeros(2 * N * (N + 1))
    load_harness().win_stitch_entries(F, _vp(np.ascontiguousarray(acc, dtype=np.float64)), _vp(adH), _vp(adT), _vp(out))
    return out[:N * N].reshape(N, N), out[N * N:N * N + N], out[N * N + N:2 * N * N + N].reshape(N, N), out[2 * N * N + N:]


def open_case(c, cls=HostWindow, **kw):
    """a window of class `cls` holding case c's parameters, calibration, frames, points and residuals"""
    w = cls(c.H, c.W, c.F, **kw)
    if c.prm:
        w.set_params(**c.prm)
    w.set_calib(*c.K)
    w.set_frames(0, c.images)
    w.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
    w.set_residuals(c.point, c.target, c.state, c.energy)
    return w


def run_rounds(w, c, copy_jacobians=True, accumulate=False):
    """linearize -> apply -> point_hessians, then the same after set_idepths(ids2): everything a caller can read, per round"""
    out = []
    for rnd in range(2):
        if rnd == 1:
            w.set_idepths(c.ids2)
        energy, counts = w.linearize(c.F, c.precalc, c.th)
        lin = w.residuals()
        w.apply(copy_jacobians)
        nres = w.point_hessians(c.prior, c.delta, c.lf, bool(c.shift))
        out.append(dict(energy=np.float64(energy), counts=counts, nres=np.int32(nres), linearized=lin, residuals=w.residuals(), points=w.points()))
        if accumulate:
            out[-1]["accumulated"] = w.accumulate(c.F, c.adH, c.adT, c.prior, c.delta, c.lf, bool(c.shift))
    return out


def dump_cases(path, cases):
    """the binary the stand-alone program reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            prm = dict(DEFAULTS)
            prm.update(c.prm)
            f.write(struct.pack("<6i", c.H, c.W, c.F, len(c.host), len(c.point), int(c.shift)) + pack_params(prm) + struct.pack("<4f", *c.K))
            for a, dt in ((c.images, "f4"), (c.host, "i4"), (c.uv, "f4"), (c.color, "f4"), (c.weights, "f4"), (c.ids, "f4"), (c.idz, "f4"),
                          (c.ids2, "f4"), (c.point, "i4"), (c.target, "i4"), (c.state, "i4"), (c.energy, "f4"), (c.precalc, "f4"), (c.th, "f4"),
                          (c.prior, "f4"), (c.delta, "f4"), (c.lf, "f4"), (c.adH, "f8"), (c.adT, "f8")):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())


def run_standalone(cases, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -g -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own hostile inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("window", SRC, "WIN_STANDALONE", extra_flags)
    dump_cases(data, cases)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/window_harness.py [g++ flags]: the sanitizer run of DESIGN §17
    import sys
    sys.path.insert(0, HERE)
    import window_cases as wc
    print(run_standalone(list(wc.cases().values()), sys.argv[1:]), end="")
