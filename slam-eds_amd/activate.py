"""ctypes binding of include/eds_hip_activate.h: the activation of DSO's immature points over an ``immature.ImmaturePoints`` — the
coarse distance map, the candidate rule and the Gauss-Newton fit of every chosen point's inverse depth, on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_activate.hip); there is no CPU fallback.
``Activation`` borrows the ``eds_imm`` of its ``ImmaturePoints``.  ``distance_precalc`` and ``precalc`` form the caller's matrices the
way DSO does; ``next_min_act_dist`` is the three comparisons of the currentMinActDist controller, which stay on the host.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi
from . import immature

(NONE, DELETED_UNTRACED, DELETED_CANNOT, KEPT_CANNOT, DELETED_OUT_OF_MAP, CHOSEN, KEPT_TOO_CLOSE, KEPT_WEAK, DROPPED, ACTIVATED) = range(10)   # eds_act_fate
FATE_NAMES = ("NONE", "DELETED_UNTRACED", "DELETED_CANNOT", "KEPT_CANNOT", "DELETED_OUT_OF_MAP", "CHOSEN", "KEPT_TOO_CLOSE", "KEPT_WEAK", "DROPPED",
              "ACTIVATED")
NUM_FATES = 10
MAX_FRAMES = 64
PRECALC_FLOATS = 14
ST_IN, ST_OOB, ST_OUTLIER = 0, 1, 2


class Params(capi.ParamStruct):
    """``eds_act_params`` — the setting_* values the activation reads."""
    _fields_ = [("min_idepth_h_act", C.c_float), ("gn_its_on_point_activation", C.c_int32), ("min_trace_quality", C.c_float),
                ("max_trace_pixel_interval", C.c_float), ("min_obs", C.c_int32), ("scale_idepth", C.c_float)]


@functools.lru_cache(maxsize=None)
def _lib():
    vp, f = C.c_void_p, C.c_float
    return capi.bind(capi.ACT_EXPORTS, {
        "eds_act_params_default": ([C.POINTER(Params)], None),
        "eds_act_set_params": [vp, C.POINTER(Params)],
        "eds_act_get_params": [vp, C.POINTER(Params)],
        "eds_act_set_calib": [vp, f, f, f, f],
        "eds_act_make_distance_map": [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int],
        "eds_act_get_distance_map": [vp, vp],
        "eds_act_select": [vp, C.c_int, C.c_int, vp, vp, vp, f, vp],
        "eds_act_optimize": [vp, C.c_int, vp, vp],
        "eds_act_get": [vp, C.c_int] + [vp] * 7,
        "eds_act_get_activated": [vp, C.c_int, C.POINTER(C.c_int)] + [vp] * 8,
    })


def default_params(**over) -> Params:
    p = Params()
    _lib().eds_act_params_default(C.byref(p))
    return p.update(**over)


def _k3(K):
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (4,):
        K = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    return K


def distance_precalc(K, T_newest_host):
    """``KRKi1`` and ``Kt1`` of one host as makeDistanceMap forms them: K[1] * R * Ki[0] and K[1] * t in fp32, with makeK's level-1
    values (fx / 2, (cx + 0.5) / 2 - 0.5) and Ki[0] the fp32 inverse of K[0].  T_newest_host is hostToNewest (3 x 4 or 4 x 4)."""
    K0 = _k3(K)
    K1 = np.array([[K0[0, 0] * 0.5, 0, (K0[0, 2] + 0.5) / 2 - 0.5], [0, K0[1, 1] * 0.5, (K0[1, 2] + 0.5) / 2 - 0.5], [0, 0, 1]], dtype=np.float32)
    Ki0 = np.linalg.inv(K0).astype(np.float32)
    T = np.asarray(T_newest_host, dtype=np.float64)
    R32, t32 = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    return ((K1 @ R32) @ Ki0).astype(np.float32), (K1 @ t32).astype(np.float32)


def precalc(T_host, T_target, aff_host=(0.0, 0.0), aff_target=(0.0, 0.0), exposures=(1.0, 1.0)):
    """One record of ``eds_act_optimize``'s precalc (14 floats): PRE_RTll, PRE_tTll and PRE_aff_mode of ``FrameFramePrecalc::set`` — the
    NON-_0 values, from the current worldToCam poses in fp64, narrowed."""
    Th, Tt = (np.vstack([np.asarray(T, dtype=np.float64)[:3], [0, 0, 0, 1.0]]) for T in (T_host, T_target))
    ll = Tt @ np.linalg.inv(Th)
    eh, et = (float(x) for x in exposures)
    if eh == 0 or et == 0:
        eh = et = 1.0
    a = np.exp(float(aff_target[0]) - float(aff_host[0])) * et / eh
    b = float(aff_target[1]) - a * float(aff_host[1])
    return np.concatenate([ll[:3, :3].ravel(), ll[:3, 3], [a, b]]).astype(np.float32)


def next_min_act_dist(n_points, desired_density, cur):
    """A currentMinActDist controller in the manner of DSO's activatePointsMT, which is not in the reference tree: fewer points than
    desired lower the distance, more raise it, clamped to 0 .. 4.  A few comparisons that stay on the host."""
    cur = float(cur)
    for frac, d in ((0.66, -0.8), (0.8, -0.5), (0.9, -0.2), (1.0, -0.1)):
        if n_points < desired_density * frac:
            cur += d
            break
    else:
        for frac, d in ((1.5, 0.8), (1.3, 0.5), (1.15, 0.2), (1.0, 0.1)):
            if n_points > desired_density * frac:
                cur += d
                break
    return min(4.0, max(0.0, cur))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


_vp = capi.vp


class Activation:
    """The activation state of an ``immature.ImmaturePoints``; it lives and dies with that object."""

    def __init__(self, points: immature.ImmaturePoints, fx=None, fy=None, cx=None, cy=None, **params):
        self.points = points
        self.n_hosts = 0
        _lib()
        if params:
            self.set_params(**params)
        if fx is not None:
            self.set_calib(fx, fy, cx, cy)

    @property
    def _h(self):
        return self.points._h

    def set_params(self, **over):
        p = self.params().update(**over)
        capi._check(_lib().eds_act_set_params(self._h, C.byref(p)))

    def params(self) -> Params:
        p = Params()
        capi._check(_lib().eds_act_get_params(self._h, C.byref(p)))
        return p

    def set_calib(self, fx, fy, cx, cy):
        capi._check(_lib().eds_act_set_calib(self._h, fx, fy, cx, cy))

    @property
    def map_shape(self):
        return self.points.H >> 1, self.points.W >> 1

    def make_distance_map(self, newest, KRKi1, Kt1, active_host=None, active_uv_idepth=None):
        """active points: numpy arrays (n ints, n x 3 floats), or two device arrays (``capi.DeviceArray`` and the like)"""
        k, t = _f32(KRKi1).reshape(-1, 9), _f32(Kt1).reshape(-1, 3)
        if len(k) != len(t):
            raise ValueError("one KRKi1 and Kt1 per host")
        if active_host is None or (not capi.is_device_source(active_host) and len(active_host) == 0):
            capi._check(_lib().eds_act_make_distance_map(self._h, int(newest), len(k), _vp(k), _vp(t), 0, None, None, 0))
            return
        if capi.is_device_source(active_host):
            hp, hs, _, hd = capi.device_array_info(active_host)
            ap, ash, _, ad = capi.device_array_info(active_uv_idepth)
            if hd != np.int32 or ad != np.float32 or int(np.prod(ash)) != 3 * int(np.prod(hs)):
                raise ValueError("device active points: int32 hosts and float32 n x 3 rows")
            capi._check(_lib().eds_act_make_distance_map(self._h, int(newest), len(k), _vp(k), _vp(t), int(np.prod(hs)), C.c_void_p(hp), C.c_void_p(ap), 1))
            return
        ah = np.ascontiguousarray(active_host, dtype=np.int32).reshape(-1)
        ac = _f32(active_uv_idepth).reshape(-1, 3)
        if len(ah) != len(ac):
            raise ValueError("one host per active point")
        capi._check(_lib().eds_act_make_distance_map(self._h, int(newest), len(k), _vp(k), _vp(t), len(ah), _vp(ah), _vp(ac), 0))

    def distance_map(self):
        out = np.zeros(self.map_shape, np.float32)
        capi._check(_lib().eds_act_get_distance_map(self._h, _vp(out)))
        return out

    def select(self, newest, KRKi1, Kt1, flagged_for_marginalization=None, current_min_act_dist=2.0):
        """the candidate rule; returns the live points per fate"""
        k, t = _f32(KRKi1).reshape(-1, 9), _f32(Kt1).reshape(-1, 3)
        if len(k) != len(t):
            raise ValueError("one KRKi1 and Kt1 per host")
        fl = None if flagged_for_marginalization is None else np.ascontiguousarray(flagged_for_marginalization, dtype=np.uint8).reshape(len(k))
        counts = np.zeros(NUM_FATES, np.int32)
        capi._check(_lib().eds_act_select(self._h, int(newest), len(k), _vp(k), _vp(t), _vp(fl), float(current_min_act_dist), _vp(counts)))
        self.n_hosts = len(k)
        return counts

    def optimize(self, precalc):
        """the fit of every CHOSEN point; precalc is F x F x 14; returns the points per fate"""
        pc = _f32(precalc).reshape(-1, PRECALC_FLOATS)
        F = int(round(len(pc) ** 0.5))
        if F * F != len(pc):
            raise ValueError("precalc is F x F x 14")
        counts = np.zeros(NUM_FATES, np.int32)
        capi._check(_lib().eds_act_optimize(self._h, F, _vp(pc), _vp(counts)))
        return counts

    def get(self, host):
        """fate, idepth, energy, hdd, bd, res_state and res_energy (n x n_hosts) per point of ``host``"""
        n, F = self.points.num_points(host), self.n_hosts
        o = dict(fate=np.zeros(n, np.int32), idepth=np.zeros(n, np.float32), energy=np.zeros(n, np.float32), hdd=np.zeros(n, np.float32),
                 bd=np.zeros(n, np.float32), res_state=np.zeros((n, F), np.int32), res_energy=np.zeros((n, F), np.float32))
        capi._check(_lib().eds_act_get(self._h, int(host), *[_vp(v) for v in o.values()]))
        return o

    def activated(self):
        """the ACTIVATED points in (host, index) order"""
        n = C.c_int()
        capi._check(_lib().eds_act_get_activated(self._h, 0, C.byref(n), *([None] * 8)))
        m = n.value
        o = dict(host=np.zeros(m, np.int32), index=np.zeros(m, np.int32), uv=np.zeros((m, 2), np.float32), type=np.zeros(m, np.float32),
                 idepth=np.zeros(m, np.float32), color=np.zeros((m, 8), np.float32), weights=np.zeros((m, 8), np.float32),
                 target_mask=np.zeros(m, np.uint64))
        capi._check(_lib().eds_act_get_activated(self._h, m, C.byref(n), *[_vp(v) for v in o.values()]))
        return o

    def window_tables(self):
        """what ``Window.set_points`` and ``Window.set_residuals`` take: one point row per activated point, one residual per IN target
        with state IN and energy 0"""
        a = self.activated()
        pt, tg = [], []
        for i, mask in enumerate(a["target_mask"]):
            for t in range(self.n_hosts):
                if (int(mask) >> t) & 1:
                    pt.append(i)
                    tg.append(t)
        m = len(pt)
        points = dict(host=a["host"], uv=a["uv"], color=a["color"], weights=a["weights"], idepth_scaled=a["idepth"], idepth_zero_scaled=a["idepth"])
        residuals = dict(point=np.array(pt, np.int32), target=np.array(tg, np.int32), state=np.zeros(m, np.int32), energy=np.zeros(m, np.float32))
        return points, residuals
