"""ctypes binding of include/eds_hip_winsolve.h: the rest of one Gauss-Newton iteration of DSO's window optimiser over a ``Window`` —
``fixLinearizationF``, ``solveSystemF`` with the point step, ``setIdepth``, ``calcLEnergyF_MT``, ``calcMEnergyF`` and the arithmetic of
``marginalizePointsF`` — on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_winsolve.hip); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi
from .window import _f32, _lib as _win_lib, _vp

SOLVER_SVD, SOLVER_ORTHOGONALIZE_SYSTEM, SOLVER_ORTHOGONALIZE_POINTMARG, SOLVER_ORTHOGONALIZE_FULL, SOLVER_SVD_CUT7 = 1, 2, 4, 8, 16
SOLVER_REMOVE_POSEPRIOR, SOLVER_USE_GN, SOLVER_FIX_LAMBDA, SOLVER_ORTHOGONALIZE_X, SOLVER_MOMENTUM, SOLVER_STEPMOMENTUM = 32, 64, 128, 256, 512, 1024
SOLVER_ORTHOGONALIZE_X_LATER = 2048
SOLVER_DEFAULT = SOLVER_FIX_LAMBDA | SOLVER_ORTHOGONALIZE_X_LATER          # reference src/utils/settings.cpp

# eds_wsv_out: name, dtype, shape as a function of (m, n, F, N)
OUT_FIELDS = (("adHTdeltaF", "f4", lambda m, n, F, N: (F * F, 8)), ("is_linearized", "i4", lambda m, n, F, N: (m,)),
              ("res_toZeroF", "f4", lambda m, n, F, N: (m, 8)), ("resApprox", "f4", lambda m, n, F, N: (m, 8)), ("lf", "f4", lambda m, n, F, N: (n, 6)),
              ("HFinal", "f8", lambda m, n, F, N: (N, N)), ("bFinal", "f8", lambda m, n, F, N: (N,)), ("xAd", "f4", lambda m, n, F, N: (F * F, 8)),
              ("frame_step", "f8", lambda m, n, F, N: (N,)), ("step", "f4", lambda m, n, F, N: (n,)), ("idepth_scaled", "f4", lambda m, n, F, N: (n,)),
              ("priorF", "f4", lambda m, n, F, N: (n,)))
SYSTEM_FIELDS = ("HFinal", "bFinal", "xAd", "frame_step")                   # need a solve


class Stats(C.Structure):
    """``eds_wsv_stats``"""
    _fields_ = [("res_in_a", C.c_int32), ("res_in_l", C.c_int32), ("orthogonalized_x", C.c_int32), ("orthogonalized_system", C.c_int32),
                ("lambda_", C.c_double)]


class Out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in OUT_FIELDS]


@functools.lru_cache(maxsize=None)
def _lib():
    _win_lib()
    vp, d, f, i = C.c_void_p, C.c_double, C.c_float, C.c_int
    return capi.bind(capi.WSV_EXPORTS, {
        "eds_wsv_set_state": [vp, i] + [vp] * 9,
        "eds_wsv_fix_linearization": [vp, vp],
        "eds_wsv_solve": [vp, i, d, i, i, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)],
        "eds_wsv_backup_idepths": [vp],
        "eds_wsv_step_idepths": [vp, f],
        "eds_wsv_get_steps": [vp, vp],
        "eds_wsv_l_energy": [vp, vp],
        "eds_wsv_m_energy": [vp, vp, vp, vp],
        "eds_wsv_marginalize_points": [vp, vp, f, d, vp, vp, vp],
        "eds_wsv_get": [vp, C.POINTER(Out)],
    })


def _f64(a, shape):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(shape)


class WindowSolver:
    """The solve, the point step, the energies and the point marginalisation of the window `win` (a ``window.Window``), which keeps
    owning the device memory; this object holds no state of its own."""

    def __init__(self, win):
        self.win = win
        self.F = 0
        _lib()

    @property
    def N(self):
        return 4 + 8 * self.F

    def set_state(self, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta, priorF=None, deltaF=None):
        F = int(F)
        adH, adT = _f64(adHost, (F * F, 8, 8)), _f64(adTarget, (F * F, 8, 8))
        de, pr, dp = _f64(delta, (F, 8)), _f64(prior, (F, 8)), _f64(delta_prior, (F, 8))
        cp, cd = _f64(cPrior, (4,)), _f64(cDelta, (4,))
        pf = None if priorF is None else _f32(priorF, (self.win.n,))
        df = None if deltaF is None else _f32(deltaF, (self.win.n,))
        capi._check(_lib().eds_wsv_set_state(self.win._h, F, _vp(adH), _vp(adT), _vp(de), _vp(pr), _vp(dp), _vp(cp), _vp(cd), _vp(pf), _vp(df)))
        self.F = F

    def fix_linearization(self, select):
        sel = np.ascontiguousarray(select, dtype=np.int32).reshape(self.win.m)
        capi._check(_lib().eds_wsv_fix_linearization(self.win._h, _vp(sel)))

    def solve(self, iteration, lam, HM, bM, mode=SOLVER_DEFAULT, have_first_frame=True, projector=None):
        """dict(x, lastHS, lastbS, res_in_a, res_in_l, lam, orthogonalized_x, orthogonalized_system); raises EdsError(ERR_NOT_USABLE)
        when x is not finite"""
        N = self.N
        hm, bm = _f64(HM, (N, N)), _f64(bM, (N,))
        P = None if projector is None else _f64(projector, (N, N))
        out = dict(x=np.zeros(N), lastHS=np.zeros((N, N)), lastbS=np.zeros(N))
        st = Stats()
        capi._check(_lib().eds_wsv_solve(self.win._h, int(iteration), float(lam), int(mode), 1 if have_first_frame else 0, _vp(hm), _vp(bm), _vp(P),
                                         _vp(out["x"]), _vp(out["lastHS"]), _vp(out["lastbS"]), C.byref(st)))
        out.update(res_in_a=st.res_in_a, res_in_l=st.res_in_l, lam=st.lambda_, orthogonalized_x=st.orthogonalized_x,
                   orthogonalized_system=st.orthogonalized_system)
        return out

    def backup_idepths(self):
        capi._check(_lib().eds_wsv_backup_idepths(self.win._h))

    def step_idepths(self, fac=1.0):
        capi._check(_lib().eds_wsv_step_idepths(self.win._h, float(fac)))

    def steps(self):
        out = np.zeros(self.win.n, np.float32)
        capi._check(_lib().eds_wsv_get_steps(self.win._h, _vp(out)))
        return out

    def l_energy(self):
        e = C.c_double()
        capi._check(_lib().eds_wsv_l_energy(self.win._h, C.cast(C.byref(e), C.c_void_p)))
        return e.value

    def m_energy(self, HM, bM):
        N = self.N
        e = C.c_double()
        capi._check(_lib().eds_wsv_m_energy(self.win._h, _vp(_f64(HM, (N, N))), _vp(_f64(bM, (N,))), C.cast(C.byref(e), C.c_void_p)))
        return e.value

    def marginalize_points(self, marg, HM, bM, prior_fac=1.0, weight_fac=1.0):
        """returns (HM, bM, res_in_m): new arrays, the caller's are not touched"""
        N = self.N
        sel = np.ascontiguousarray(marg, dtype=np.int32).reshape(self.win.n)
        hm, bm = _f64(HM, (N, N)).copy(), _f64(bM, (N,)).copy()
        res = C.c_int32()
        capi._check(_lib().eds_wsv_marginalize_points(self.win._h, _vp(sel), float(prior_fac), float(weight_fac), _vp(hm), _vp(bm),
                                                      C.cast(C.byref(res), C.c_void_p)))
        return hm, bm, res.value

    def get(self, system=True):
        """everything eds_wsv_get reads back; system = False leaves out what needs a solve"""
        m, n, F, N = self.win.m, self.win.n, self.F, self.N
        out = {k: np.zeros(sh(m, n, F, N), dt) for k, dt, sh in OUT_FIELDS if system or k not in SYSTEM_FIELDS}
        o = Out(**{k: out[k].ctypes.data for k in out})
        capi._check(_lib().eds_wsv_get(self.win._h, C.byref(o)))
        return out
