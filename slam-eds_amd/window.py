"""ctypes binding of include/eds_hip_window.h: the per-residual and per-point part of DSO's window optimiser —
``PointFrameResidual::linearize`` over every residual of the window, ``applyRes`` with ``takeDataF``, the per-point sums of the active
top Hessian and the Schur complement's per-point prologue — on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_window.hip); there is no CPU fallback.  ``Window`` owns
one ``eds_win``.  ``precalc`` forms ``FrameFramePrecalc::set``'s fp32 values; ``adjoints`` is ``setAdjointsF`` in numpy for the caller's stitch.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi

MAX_FRAMES, PRECALC_FLOATS, J_WORDS = 8, 27, 74                 # EDS_WIN_MAX_FRAMES, EDS_WIN_PRECALC_FLOATS, EDS_WIN_J_WORDS
IN, OOB, OUTLIER = 0, 1, 2

# eds_win_residual_out and eds_win_point_out: name, dtype, trailing shape
RESIDUAL_FIELDS = (("state", "i4", ()), ("energy", "f4", ()), ("new_state", "i4", ()), ("new_energy", "f4", ()),
                   ("new_energy_with_outlier", "f4", ()), ("linearize_return", "f4", ()), ("is_active", "i4", ()),
                   ("center_projected_to", "f4", (3,)), ("projected_to", "f4", (8, 2)), ("J", "f4", (J_WORDS,)), ("ef_J", "f4", (J_WORDS,)),
                   ("JpJdF", "f4", (8,)))
POINT_FIELDS = (("Hdd_accAF", "f4", ()), ("bd_accAF", "f4", ()), ("Hcd_accAF", "f4", (4,)), ("HdiF", "f4", ()), ("bdSumF", "f4", ()),
                ("idepth_hessian", "f4", ()), ("nres", "i4", ()))


class Params(capi.ParamStruct):
    """``eds_win_params`` — the setting_* values and SCALE_* constants linearize reads (settings.cpp:91-127, HessianBlocks.h:58-62)."""
    _fields_ = [("outlier_th_sum_component", C.c_float), ("huber_th", C.c_float), ("affine_opt_mode_a", C.c_float),
                ("affine_opt_mode_b", C.c_float), ("scale_idepth", C.c_float), ("scale_f", C.c_float), ("scale_c", C.c_float),
                ("reserved", C.c_float)]


class ResidualOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in RESIDUAL_FIELDS]


class PointOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in POINT_FIELDS]


@functools.lru_cache(maxsize=None)
def _lib():
    vp, i64, f = C.c_void_p, C.c_int64, C.c_float
    return capi.bind(capi.WIN_EXPORTS, {
        "eds_win_params_default": ([C.POINTER(Params)], None),
        "eds_win_create": [C.c_int] * 6 + [C.POINTER(vp)],
        "eds_win_destroy": ([vp], None),
        "eds_win_set_params": [vp, C.POINTER(Params)],
        "eds_win_get_params": [vp, C.POINTER(Params)],
        "eds_win_set_calib": [vp, f, f, f, f],
        "eds_win_set_frames": [vp, C.c_int, C.c_int, vp, i64, i64, C.c_int],
        "eds_win_get_frame": [vp, C.c_int, vp],
        "eds_win_set_points": [vp, C.c_int, vp, vp, vp, vp, vp, vp],
        "eds_win_set_idepths": [vp, vp, vp],
        "eds_win_set_residuals": [vp, C.c_int, vp, vp, vp, vp],
        "eds_win_linearize": [vp, C.c_int, vp, vp, vp, vp],
        "eds_win_apply": [vp, C.c_int],
        "eds_win_point_hessians": [vp, vp, vp, vp, C.c_int, vp],
        "eds_win_get_residuals": [vp, C.POINTER(ResidualOut)],
        "eds_win_accumulate": [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp],
        "eds_win_acc_size": [C.c_int],
        "eds_win_get_points": [vp, C.POINTER(PointOut)],
    })


def default_params(**over) -> Params:
    p = Params()
    _lib().eds_win_params_default(C.byref(p))
    return p.update(**over)


def _se3(T):
    T = np.asarray(T, dtype=np.float64)
    if T.shape == (3, 4):
        T = np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]])
    if T.shape != (4, 4):
        raise ValueError("a pose is 3 x 4 or 4 x 4")
    return T


def precalc(K, T_host, T_target, T0_host=None, T0_target=None, aff_host=(0.0, 0.0), aff_target=(0.0, 0.0), exposures=(1.0, 1.0), b0_host=None):
    """One record of ``eds_win_linearize``'s precalc (27 floats) as ``FrameFramePrecalc::set`` forms it (HessianBlocks.cpp:204-234): the
    poses are worldToCam (PRE_worldToCam, and the evaluation point's for T0_*; None: the same), products and inverses in fp64, the
    rotation and translation narrowed to fp32, K R K^-1 and K t in fp32; the affine pair is AffLight::fromToVecExposure in fp64,
    narrowed; b0 is the host's aff_g2l_0().b (None: aff_host[1])."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (4,):
        K = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    K32, Ki32 = K.astype(np.float32), np.linalg.inv(K).astype(np.float32)
    Th, Tt = _se3(T_host), _se3(T_target)
    T0h, T0t = (Th if T0_host is None else _se3(T0_host)), (Tt if T0_target is None else _se3(T0_target))
    ll0, ll = T0t @ np.linalg.inv(T0h), Tt @ np.linalg.inv(Th)
    R32, t32 = ll[:3, :3].astype(np.float32), ll[:3, 3].astype(np.float32)
    eh, et = (float(x) for x in exposures)
    if eh == 0 or et == 0:
        eh = et = 1.0
    a = np.exp(float(aff_target[0]) - float(aff_host[0])) * et / eh
    b = float(aff_target[1]) - a * float(aff_host[1])
    out = np.concatenate([((K32 @ R32) @ Ki32).ravel(), K32 @ t32, ll0[:3, :3].ravel(), ll0[:3, 3], [a, b],
                          [aff_host[1] if b0_host is None else b0_host]])
    return out.astype(np.float32)


def adjoints(T_world_to_cam, aff=None, exposures=None):
    """``EnergyFunctional::setAdjointsF`` (EnergyFunctional.cpp:46-86) in numpy from the evaluation-point poses and aff_g2l_0:
    (adHost, adTarget), each F x F x 8 x 8 fp64 indexed [target][host] as the reference's h + F * t.  A convenience for the caller's stitch; no bit claim rests on it."""
    Ts = [_se3(T) for T in T_world_to_cam]
    F = len(Ts)
    aff = np.zeros((F, 2)) if aff is None else np.asarray(aff, dtype=np.float64)
    exposures = np.ones(F) if exposures is None else np.asarray(exposures, dtype=np.float64)

    def hat(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])

    adH, adT = np.zeros((F, F, 8, 8)), np.zeros((F, F, 8, 8))
    for h in range(F):
        for t in range(F):
            ll = Ts[t] @ np.linalg.inv(Ts[h])
            R, tr = ll[:3, :3], ll[:3, 3]
            Adj = np.zeros((6, 6))
            Adj[:3, :3], Adj[3:, 3:], Adj[:3, 3:] = R, R, hat(tr) @ R
            AH, AT = np.eye(8), np.eye(8)
            AH[:6, :6] = -Adj.T
            eh, et = exposures[h], exposures[t]
            if eh == 0 or et == 0:
                eh = et = 1.0
            a = float(np.float32(np.exp(aff[t, 0] - aff[h, 0]) * et / eh))
            AT[6, 6], AH[6, 6], AT[7, 7], AH[7, 7] = -a, a, -1.0, a
            for M in (AH, AT):                                  # SCALE_XI_TRANS = SCALE_XI_ROT = 1, SCALE_A = 10, SCALE_B = 1000
                M[6, :] *= 10.0
                M[7, :] *= 1000.0
            adH[t, h], adT[t, h] = AH, AT
    return adH, adT


_vp = capi.vp


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


class Window(capi.OwnedHandle):
    """The frames, points and residuals of one optimisation window in device memory."""
    _destroy = "eds_win_destroy"

    def __init__(self, H, W, max_frames=MAX_FRAMES, max_points=20000, max_residuals=140000, device=0, **params):
        self._h = C.c_void_p()
        self.H, self.W, self.max_frames, self.max_points, self.max_residuals = int(H), int(W), int(max_frames), int(max_points), int(max_residuals)
        self.n = self.m = 0
        self.device = int(device)
        capi._check(_lib().eds_win_create(int(device), self.H, self.W, self.max_frames, self.max_points, self.max_residuals, C.byref(self._h)))
        if params:
            self.set_params(**params)

    def set_params(self, **over):
        p = self.params().update(**over)
        capi._check(_lib().eds_win_set_params(self._h, C.byref(p)))

    def params(self) -> Params:
        p = Params()
        capi._check(_lib().eds_win_get_params(self._h, C.byref(p)))
        return p

    def set_calib(self, fx, fy, cx, cy):
        capi._check(_lib().eds_win_set_calib(self._h, fx, fy, cx, cy))

    def set_frames(self, first, images):
        """images: count x H x W (or one H x W) on the host, or a device array of that shape with contiguous rows"""
        if capi.is_device_source(images):
            ptr, shape, est, dt = capi.device_array_info(images)
            shape, est = tuple(shape), tuple(est)
            if len(shape) == 2:
                shape, est = (1,) + shape, (shape[0] * est[0],) + est
            if dt != np.float32 or shape[1:] != (self.H, self.W) or est[2] != 1:
                raise ValueError(f"device frames must be float32 count x {self.H} x {self.W} with contiguous rows")
            capi._check(_lib().eds_win_set_frames(self._h, int(first), shape[0], C.c_void_p(ptr), int(est[1]), int(est[0]), 1))
            return
        a = _f32(images)
        if a.ndim == 2:
            a = a[None]
        if a.shape[1:] != (self.H, self.W):
            raise ValueError(f"frames must be count x {self.H} x {self.W}, not {a.shape}")
        capi._check(_lib().eds_win_set_frames(self._h, int(first), len(a), _vp(a), 0, 0, 0))

    def frame(self, f):
        out = np.zeros((self.H, self.W, 3), np.float32)
        capi._check(_lib().eds_win_get_frame(self._h, int(f), _vp(out)))
        return out

    def set_points(self, host, uv, color, weights, idepth_scaled, idepth_zero_scaled=None):
        host = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
        n = len(host)
        uv, color, weights = _f32(uv, (n, 2)), _f32(color, (n, 8)), _f32(weights, (n, 8))
        ids = _f32(idepth_scaled, (n,))
        idz = ids if idepth_zero_scaled is None else _f32(idepth_zero_scaled, (n,))
        capi._check(_lib().eds_win_set_points(self._h, n, _vp(host), _vp(uv), _vp(color), _vp(weights), _vp(ids), _vp(idz)))
        self.n, self.m = n, 0

    def set_idepths(self, idepth_scaled=None, idepth_zero_scaled=None):
        ids = None if idepth_scaled is None else _f32(idepth_scaled, (self.n,))
        idz = None if idepth_zero_scaled is None else _f32(idepth_zero_scaled, (self.n,))
        capi._check(_lib().eds_win_set_idepths(self._h, _vp(ids), _vp(idz)))

    def set_residuals(self, point, target, state=None, energy=None):
        point = np.ascontiguousarray(point, dtype=np.int32).reshape(-1)
        m = len(point)
        target = np.ascontiguousarray(target, dtype=np.int32).reshape(m)
        st = None if state is None else np.ascontiguousarray(state, dtype=np.int32).reshape(m)
        en = None if energy is None else _f32(energy, (m,))
        capi._check(_lib().eds_win_set_residuals(self._h, m, _vp(point), _vp(target), _vp(st), _vp(en)))
        self.m = m

    def linearize(self, F, precalc, frame_energy_th):
        """returns (energy, counts of the new states IN / OOB / OUTLIER)"""
        pc = _f32(precalc, (int(F) * int(F), PRECALC_FLOATS))
        th = _f32(frame_energy_th, (int(F),))
        e, counts = C.c_double(), np.zeros(3, np.int32)
        capi._check(_lib().eds_win_linearize(self._h, int(F), _vp(pc), _vp(th), C.cast(C.byref(e), C.c_void_p), _vp(counts)))
        return e.value, counts

    def apply(self, copy_jacobians=True):
        capi._check(_lib().eds_win_apply(self._h, 1 if copy_jacobians else 0))

    def point_hessians(self, priorF=None, deltaF=None, lf=None, shift_prior_to_zero=False):
        """returns nres"""
        pr = None if priorF is None else _f32(priorF, (self.n,))
        de = None if deltaF is None else _f32(deltaF, (self.n,))
        l = None if lf is None else _f32(lf, (self.n, 6))
        nres = C.c_int32()
        capi._check(_lib().eds_win_point_hessians(self._h, _vp(pr), _vp(de), _vp(l), 1 if shift_prior_to_zero else 0, C.cast(C.byref(nres), C.c_void_p)))
        return nres.value

    def accumulate(self, F, adHost, adTarget, priorF=None, deltaF=None, lf=None, shift_prior_to_zero=False):
        """point_hessians, every accumulator of the two addPoint()s on the device, both stitches: dict(H_A, b_A, H_sc, b_sc, acc, nres);
        adHost / adTarget are indexed [h + F * t] (``adjoints`` returns them as [t][h])"""
        F = int(F)
        N = 4 + 8 * F
        adH, adT = (np.ascontiguousarray(a, dtype=np.float64).reshape(F * F, 8, 8) for a in (adHost, adTarget))
        pr = None if priorF is None else _f32(priorF, (self.n,))
        de = None if deltaF is None else _f32(deltaF, (self.n,))
        l = None if lf is None else _f32(lf, (self.n, 6))
        out = dict(H_A=np.zeros((N, N)), b_A=np.zeros(N), H_sc=np.zeros((N, N)), b_sc=np.zeros(N), acc=np.zeros(_lib().eds_win_acc_size(F)))
        nres = C.c_int32()
        capi._check(_lib().eds_win_accumulate(self._h, F, _vp(adH), _vp(adT), _vp(pr), _vp(de), _vp(l), 1 if shift_prior_to_zero else 0,
                                              _vp(out["H_A"]), _vp(out["b_A"]), _vp(out["H_sc"]), _vp(out["b_sc"]), _vp(out["acc"]),
                                              C.cast(C.byref(nres), C.c_void_p)))
        out["nres"] = np.int32(nres.value)
        return out

    def residuals(self):
        out = {k: np.zeros((self.m,) + sh, dt) for k, dt, sh in RESIDUAL_FIELDS}
        o = ResidualOut(**{k: out[k].ctypes.data for k in out})
        capi._check(_lib().eds_win_get_residuals(self._h, C.byref(o)))
        return out

    def points(self):
        out = {k: np.zeros((self.n,) + sh, dt) for k, dt, sh in POINT_FIELDS}
        o = PointOut(**{k: out[k].ctypes.data for k in out})
        capi._check(_lib().eds_win_get_points(self._h, C.byref(o)))
        return out
