"""ctypes binding of include/eds_hip_winflag.h: each point's residual history (``numGoodResiduals``, ``maxRelBaseline``,
``lastResiduals``, and ``isNew`` per residual) kept on the device beside a ``Window``, travelling with every edit of
``winedit.WindowEdit``; ``makeKeyFrame``'s residuals towards a new keyframe, and the ``fixLinearization`` half of ``linearizeAll``.

Plumbing only: the columns are written by the HIP kernels behind the C ABI (csrc/eds_winflag.hip); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi
from .window import _vp
from .winedit import _lib as _wed_lib

# eds_wfl_history: name, dtype, shape as a function of (m, n)
HISTORY_FIELDS = (("num_good", "i4", lambda m, n: (n,)), ("max_rel_baseline", "f4", lambda m, n: (n,)), ("last_target", "i4", lambda m, n: (n, 2)),
                  ("last_state", "i4", lambda m, n: (n, 2)), ("is_new", "i4", lambda m, n: (m,)))


KEEP, MARGINALIZE, DROP = 0, 1, 2


class Params(capi.ParamStruct):
    _fields_ = [("min_good_active_res_for_marg", C.c_int32), ("min_good_res_for_marg", C.c_int32), ("min_idepth_h_marg", C.c_float), ("reserved", C.c_int32)]


class History(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in HISTORY_FIELDS]


@functools.lru_cache(maxsize=None)
def _lib():
    _wed_lib()
    vp, i = C.c_void_p, C.c_int
    return capi.bind(capi.WFL_EXPORTS, {
        "eds_wfl_set_history": [vp, C.POINTER(History), i],
        "eds_wfl_get_history": [vp, C.POINTER(History)],
        "eds_wfl_insert_frame_residuals": [vp, i, vp],
        "eds_wfl_apply_fixed": [vp, i, vp, i, vp],
        "eds_wfl_params_default": ([C.POINTER(Params)], None),
        "eds_wfl_flag_points": [vp, i, C.c_uint32, C.POINTER(Params), vp, vp, i, vp],
        "eds_wfl_get_fates": [vp, vp],
        "eds_wfl_marginalize_flagged": [vp, C.c_float, C.c_double, vp, vp, vp],
        "eds_wfl_remove_flagged": [vp, vp, vp],
    })


class WindowFlags:
    """The history of the points of `win` (a ``window.Window``), which keeps owning the device memory; `win.m` follows an insert."""

    def __init__(self, win):
        self.win = win
        _lib()

    def set_history(self, **columns):
        """the columns named (numpy arrays, or device arrays: all of one kind); every other column takes its defaults"""
        m, n = self.win.m, self.win.n
        unknown = set(columns) - {k for k, _, _ in HISTORY_FIELDS}
        if unknown:
            raise ValueError(f"no such columns: {sorted(unknown)}")
        on_device = [capi.is_device_source(v) for v in columns.values() if v is not None]
        if len(set(on_device)) > 1:
            raise ValueError("the columns are all host arrays or all device arrays")
        keep, ptrs = [], {}
        for k, dt, sh in HISTORY_FIELDS:
            v = columns.get(k)
            if v is None:
                continue
            if on_device[0]:
                ptr, shape, est, dtype = capi.device_array_info(v)
                if dtype != np.dtype(dt) or int(np.prod(shape)) != int(np.prod(sh(m, n))):
                    raise ValueError(f"{k}: a contiguous {dt} device array of shape {sh(m, n)}")
                ptrs[k] = ptr
            else:
                a = np.ascontiguousarray(v, dtype=dt).reshape(sh(m, n))
                ptrs[k] = a.ctypes.data
                keep.append(a)
            keep.append(v)
        capi._check(_lib().eds_wfl_set_history(self.win._h, C.byref(History(**ptrs)), int(bool(on_device and on_device[0]))))

    def history(self):
        """every column read back: a dict of numpy arrays"""
        m, n = self.win.m, self.win.n
        out = {k: np.zeros(sh(m, n), dt) for k, dt, sh in HISTORY_FIELDS}
        capi._check(_lib().eds_wfl_get_history(self.win._h, C.byref(History(**{k: v.ctypes.data for k, v in out.items()}))))
        return out

    def insert_frame_residuals(self, frame):
        """every point not hosted by `frame` and without a residual towards it gets one, at the end of its run; returns how many"""
        inserted = C.c_int32()
        capi._check(_lib().eds_wfl_insert_frame_residuals(self.win._h, int(frame), C.cast(C.byref(inserted), C.c_void_p)))
        self.win.m += inserted.value
        return inserted.value

    def apply_fixed(self, F, precalc, clear_is_new=False):
        """``applyRes(true)`` and the history's update after a ``linearize``; returns the residuals now (IN, OOB, OUTLIER)"""
        F = int(F)
        pc = np.ascontiguousarray(precalc, dtype=np.float32).reshape(F * F, 27)
        counts = np.zeros(3, np.int32)
        capi._check(_lib().eds_wfl_apply_fixed(self.win._h, F, _vp(pc), int(bool(clear_is_new)), _vp(counts)))
        return counts

    def flag_points(self, F, frames_to_marg, precalc, frame_energy_th, only_empty=False, **params):
        """``flagPointsForRemoval`` (``only_empty``: ``removeOutliers``' point loop); `frames_to_marg`: the frames flagged for
        marginalisation (an iterable of indices, or the bit mask).  Returns (kept, marginalised, dropped) and the same per host [8, 3];
        the fates stay on the device"""
        F = int(F)
        mask = frames_to_marg if isinstance(frames_to_marg, (int, np.integer)) else sum(1 << int(f) for f in set(frames_to_marg))
        prm = Params()
        _lib().eds_wfl_params_default(C.byref(prm))
        prm.update(**params)
        pc = np.ascontiguousarray(precalc, dtype=np.float32).reshape(F * F, 27)
        th = np.ascontiguousarray(frame_energy_th, dtype=np.float32).reshape(F)
        counts = np.zeros(27, np.int32)
        capi._check(_lib().eds_wfl_flag_points(self.win._h, F, int(mask), C.byref(prm), _vp(pc), _vp(th), int(bool(only_empty)), _vp(counts)))
        return counts[:3].copy(), counts[3:].reshape(8, 3).copy()

    def fates(self):
        out = np.zeros(self.win.n, np.int32)
        capi._check(_lib().eds_wfl_get_fates(self.win._h, _vp(out)))
        return out

    def marginalize_flagged(self, HM, bM, prior_fac=1.0, weight_fac=1.0):
        """``eds_wsv_marginalize_points`` for the points with fate MARGINALIZE: returns (HM, bM, residuals in the marginalisation)"""
        bm = np.array(bM, dtype=np.float64).reshape(-1)
        hm = np.array(HM, dtype=np.float64).reshape(len(bm), len(bm))
        res = C.c_int32()
        capi._check(_lib().eds_wfl_marginalize_flagged(self.win._h, float(prior_fac), float(weight_fac), _vp(hm), _vp(bm), C.cast(C.byref(res), C.c_void_p)))
        return hm, bm, res.value

    def remove_flagged(self):
        """``eds_wed_remove_points`` for the points whose fate is not KEEP; returns (points removed, residuals removed)"""
        rp, rr = C.c_int32(), C.c_int32()
        capi._check(_lib().eds_wfl_remove_flagged(self.win._h, C.cast(C.byref(rp), C.c_void_p), C.cast(C.byref(rr), C.c_void_p)))
        self.win.n -= rp.value
        self.win.m -= rr.value
        return rp.value, rr.value
