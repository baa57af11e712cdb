"""ctypes binding of include/eds_hip_winedit.h: the window's tables edited on the device — ``dropResidual`` for a selection of
residuals, ``dropPointsF`` / ``removePoint`` for a selection of points, ``marginalizeFrame`` with the frame's removal, and ``setDeltaF``
from the device's inverse depths — so that a ``Window`` keeps its rows (Jacobians, linearized flags, L sums, steps, backups) across a
point marginalisation, an outlier removal or a keyframe change instead of being read back and set again.

Plumbing only: every row is moved by the HIP kernels behind the C ABI (csrc/eds_winedit.hip); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi
from .window import _vp
from .winsolve import _lib as _wsv_lib

# eds_wed_out: name, dtype, shape as a function of (m, n)
OUT_FIELDS = (("point", "i4", lambda m, n: (m,)), ("target", "i4", lambda m, n: (m,)), ("res_first", "i4", lambda m, n: (n + 1,)),
              ("host", "i4", lambda m, n: (n,)), ("uv", "f4", lambda m, n: (n, 2)), ("color", "f4", lambda m, n: (n, 8)),
              ("weights", "f4", lambda m, n: (n, 8)), ("idepth_zero_scaled", "f4", lambda m, n: (n,)), ("deltaF", "f4", lambda m, n: (n,)),
              ("idepth_backup", "f4", lambda m, n: (n,)))
STATE_FIELDS = ("idepth_backup",)                                # need an eds_wsv state to have been set once


class Out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _, _ in OUT_FIELDS]


@functools.lru_cache(maxsize=None)
def _lib():
    _wsv_lib()
    vp, i = C.c_void_p, C.c_int
    return capi.bind(capi.WED_EXPORTS, {
        "eds_wed_remove_residuals": [vp, vp, i, vp],
        "eds_wed_remove_points": [vp, vp, i, vp, vp],
        "eds_wed_marginalize_frame": [vp, i, vp, vp, vp, vp, vp, vp],
        "eds_wed_insert_activated": [vp, vp, vp, vp],
        "eds_wed_set_state": [vp, i] + [vp] * 7,
        "eds_wed_counts": [vp, vp, vp, vp],
        "eds_wed_get": [vp, C.POINTER(Out)],
    })


def _flags(flags, count):
    """(pointer, on_device, keep-alive) of `count` int32 flags: a numpy array (anything array-like), or a device array
    (``__cuda_array_interface__`` or a raw (ptr, shape, strides, dtype) tuple) that is contiguous int32"""
    if capi.is_device_source(flags):
        ptr, shape, est, dt = capi.device_array_info(flags)
        if dt != np.int32 or tuple(shape) != (count,) or (count > 1 and tuple(est) != (1,)):
            raise ValueError(f"device flags must be {count} contiguous int32 values")
        return C.c_void_p(ptr), 1, flags
    a = np.ascontiguousarray(flags, dtype=np.int32).reshape(count)
    return _vp(a), 0, a


class WindowEdit:
    """The edits of the window `win` (a ``window.Window``), which keeps owning the device memory; `win.n` / `win.m` follow every edit,
    and so does the `F` of `solver` (a ``winsolve.WindowSolver`` over the same window) when one is given."""

    def __init__(self, win, solver=None):
        self.win, self.solver = win, solver
        _lib()

    def marginalize_frame(self, frame, prior, delta_prior, HM, bM):
        """``marginalizeFrame`` and the frame's removal: returns (HM', bM') of size N - 8; the eds_wsv state is invalid afterwards"""
        bm = np.ascontiguousarray(bM, dtype=np.float64).reshape(-1)
        N = len(bm)
        hm = np.ascontiguousarray(HM, dtype=np.float64).reshape(N, N)
        pr, dp = (np.ascontiguousarray(a, dtype=np.float64).reshape(8) for a in (prior, delta_prior))
        out_h, out_b = np.zeros((max(N - 8, 0), max(N - 8, 0))), np.zeros(max(N - 8, 0))
        capi._check(_lib().eds_wed_marginalize_frame(self.win._h, int(frame), _vp(pr), _vp(dp), _vp(hm), _vp(bm), _vp(out_h), _vp(out_b)))
        self.win.n, self.win.m, _ = self.counts()
        return out_h, out_b

    def set_state(self, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta):
        """``eds_wsv_set_state`` with priorF kept and deltaF formed from the device's inverse depths"""
        F = int(F)
        f64 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)      # noqa: E731
        capi._check(_lib().eds_wed_set_state(self.win._h, F, _vp(f64(adHost, (F * F, 8, 8))), _vp(f64(adTarget, (F * F, 8, 8))), _vp(f64(delta, (F, 8))),
                                             _vp(f64(prior, (F, 8))), _vp(f64(delta_prior, (F, 8))), _vp(f64(cPrior, (4,))), _vp(f64(cDelta, (4,)))))
        if self.solver is not None:
            self.solver.F = F

    def insert_activated(self, activation):
        """the ACTIVATED points of `activation` (an ``activate.Activation`` after ``optimize``) enter the window, merged per host after
        the host's own points, straight from the device; returns (points inserted, residuals inserted)"""
        ip, ir = C.c_int32(), C.c_int32()
        capi._check(_lib().eds_wed_insert_activated(self.win._h, activation._h, C.cast(C.byref(ip), C.c_void_p), C.cast(C.byref(ir), C.c_void_p)))
        self.win.n += ip.value
        self.win.m += ir.value
        return ip.value, ir.value

    def remove_residuals(self, select=None):
        """removes the residuals with select[r] != 0 (None: every residual whose state is not IN); returns how many went"""
        ptr, on_device, keep = (None, 0, None) if select is None else _flags(select, self.win.m)
        removed = C.c_int32()
        capi._check(_lib().eds_wed_remove_residuals(self.win._h, ptr, on_device, C.cast(C.byref(removed), C.c_void_p)))
        self.win.m -= removed.value
        return removed.value

    def remove_points(self, flag):
        """removes the points with flag[p] != 0 and all their residuals; returns (points removed, residuals removed)"""
        ptr, on_device, keep = _flags(flag, self.win.n)
        rp, rr = C.c_int32(), C.c_int32()
        capi._check(_lib().eds_wed_remove_points(self.win._h, ptr, on_device, C.cast(C.byref(rp), C.c_void_p), C.cast(C.byref(rr), C.c_void_p)))
        self.win.n -= rp.value
        self.win.m -= rr.value
        return rp.value, rr.value

    def counts(self):
        """(n, m, points per host frame[8])"""
        n, m, per_host = C.c_int32(), C.c_int32(), np.zeros(8, np.int32)
        capi._check(_lib().eds_wed_counts(self.win._h, C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(m), C.c_void_p), _vp(per_host)))
        return n.value, m.value, per_host

    def rows(self, state=True):
        """the rows eds_wed_get reads back; state = False leaves out what needs an eds_wsv state"""
        m, n = self.win.m, self.win.n
        out = {k: np.zeros(sh(m, n), dt) for k, dt, sh in OUT_FIELDS if state or k not in STATE_FIELDS}
        o = Out(**{k: out[k].ctypes.data for k in out})
        capi._check(_lib().eds_wed_get(self.win._h, C.byref(o)))
        return out
