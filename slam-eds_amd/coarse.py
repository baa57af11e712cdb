"""ctypes binding of include/eds_hip_coarse.h: DSO's coarse image tracker as EDS uses it for the pose of every new image frame — makeK,
every level of makeImages, setCoarseTrackingRef and the whole of ``trackNewestCoarse`` for a batch of initial guesses, on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_coarse.hip); there is no CPU fallback.
``CoarseTracker`` owns one ``eds_ct``.  ``trace_precalc`` turns a returned pose into the three arguments of ``eds_imm_trace``.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi

MAX_LEVELS, MAX_DECISIONS, MAX_POINTS = 5, 512, 65536           # EDS_CT_MAX_LEVELS, EDS_CT_MAX_DECISIONS, EDS_CT_MAX_POINTS
REF_IMAGE, NEW_IMAGE, IDEPTH, WEIGHT_SUMS, PC = range(5)


class Params(capi.ParamStruct):
    """``eds_ct_params`` — the setting_* values trackNewestCoarse reads (reference src/utils/settings.cpp:119-138)."""
    _fields_ = [("huber_th", C.c_float), ("coarse_cutoff_th", C.c_float), ("affine_opt_mode_a", C.c_float), ("affine_opt_mode_b", C.c_float)]


class Result(C.Structure):
    """``eds_ct_result`` — one try of eds_ct_track."""
    _fields_ = [("T", C.c_double * 12), ("aff", C.c_double * 2), ("last_residuals", C.c_double * 5), ("last_flow_indicators", C.c_double * 3),
                ("ok", C.c_int32), ("n_decisions", C.c_int32), ("iterations", C.c_int32 * 5), ("accepts", C.c_int32 * 5),
                ("level_cutoff_repeat", C.c_float), ("reserved", C.c_int32), ("decisions", C.c_uint8 * MAX_DECISIONS)]


# eds_ct_result and eds_ct_row as numpy records
RESULT = np.dtype([("T", "f8", (3, 4)), ("aff", "f8", 2), ("last_residuals", "f8", 5), ("last_flow_indicators", "f8", 3), ("ok", "i4"),
                   ("n_decisions", "i4"), ("iterations", "i4", 5), ("accepts", "i4", 5), ("level_cutoff_repeat", "f4"), ("reserved", "i4"),
                   ("decisions", "u1", MAX_DECISIONS)])
ROW = np.dtype([("in_e", "i4"), ("warped", "i4"), ("flow", "i4"), ("energy", "f4"), ("idepth", "f4"), ("u", "f4"), ("v", "f4"), ("dx", "f4"),
                ("dy", "f4"), ("residual", "f4"), ("weight", "f4"), ("ref_color", "f4"), ("shift_t_pos", "f4"), ("shift_t_neg", "f4"),
                ("shift_rt_pos", "f4"), ("shift_rt_neg", "f4")])
assert RESULT.itemsize == C.sizeof(Result) and ROW.itemsize == 64


@functools.lru_cache(maxsize=None)
def _lib():
    vp, i64, f, d = C.c_void_p, C.c_int64, C.c_float, C.c_double
    return capi.bind(capi.CT_EXPORTS, {
        "eds_ct_params_default": ([C.POINTER(Params)], None),
        "eds_ct_create": [C.c_int] * 6 + [C.POINTER(vp)],
        "eds_ct_destroy": ([vp], None),
        "eds_ct_set_params": [vp, C.POINTER(Params)],
        "eds_ct_get_params": [vp, C.POINTER(Params)],
        "eds_ct_set_calib": [vp, f, f, f, f],
        "eds_ct_get_k": [vp, C.c_int, vp],
        "eds_ct_set_ref": [vp, vp, i64, C.c_int, f, d, d, C.c_int, vp, vp, vp, vp],
        "eds_ct_set_new": [vp, vp, i64, C.c_int, f],
        "eds_ct_track": [vp, C.c_int, vp, vp, C.c_int, vp, vp],
        "eds_ct_calc_res": [vp, C.c_int, vp, vp, f, vp, vp, vp, vp],
        "eds_ct_get_level": [vp, C.c_int, C.c_int, vp, vp],
    })


def default_params(**over) -> Params:
    p = Params()
    _lib().eds_ct_params_default(C.byref(p))
    return p.update(**over)


def trace_precalc(K, T, aff_host, aff_target, exposures=(1.0, 1.0)):
    """``eds_imm_trace``'s KRKi, Kt and affine pair from a pose this tracker returned: T is hostToNew as 3 x 4 [R | t] (for the
    reference keyframe itself, ``result["T"]``; for another host, that times the host's pose relative to the keyframe)."""
    from . import immature
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    return immature.precalc(K, T[:, :3], T[:, 3], aff_host, aff_target, exposures)


_vp = capi.vp


class CoarseTracker(capi.OwnedHandle):
    """One reference keyframe with its coarse depth, one new frame, and the alignment of the two, in device memory."""
    _destroy = "eds_ct_destroy"

    def __init__(self, H, W, levels=5, max_points=20000, max_tries=8, device=0, **params):
        self._h = C.c_void_p()
        self.H, self.W, self.levels, self.max_points, self.max_tries, self.device = int(H), int(W), int(levels), int(max_points), int(max_tries), int(device)
        capi._check(_lib().eds_ct_create(self.device, self.H, self.W, self.levels, self.max_points, self.max_tries, C.byref(self._h)))
        self.pc_n = np.zeros(self.levels, np.int32)
        if params:
            self.set_params(**params)

    def set_params(self, **over):
        p = self.params().update(**over)
        capi._check(_lib().eds_ct_set_params(self._h, C.byref(p)))

    def params(self) -> Params:
        p = Params()
        capi._check(_lib().eds_ct_get_params(self._h, C.byref(p)))
        return p

    def set_calib(self, fx, fy, cx, cy):
        capi._check(_lib().eds_ct_set_calib(self._h, fx, fy, cx, cy))

    def K(self, lvl):
        out = np.zeros(4, np.float32)
        capi._check(_lib().eds_ct_get_k(self._h, int(lvl), _vp(out)))
        return out

    def _image(self, image):
        """(pointer, row stride in elements, on_device, keep-alive)"""
        if not capi.is_device_source(image):
            a = np.ascontiguousarray(image, dtype=np.float32)
            if a.shape != (self.H, self.W):
                raise ValueError(f"image must be {self.H} x {self.W}, not {a.shape}")
            return a.ctypes.data_as(C.c_void_p), 0, 0, a
        ptr, shape, est, dt = capi.device_array_info(image)
        if dt != np.float32 or tuple(shape) != (self.H, self.W) or est[1] != 1:
            raise ValueError(f"a device image must be float32 {self.H} x {self.W} with contiguous rows")
        return C.c_void_p(ptr), int(est[0]), 1, image

    def set_ref(self, image, center_projected, hdif, exposure=1.0, aff=(0.0, 0.0)):
        """the reference frame and its contributions (n x 3 centerProjectedTo, n HdiF); returns (pc_n per level, dropped)"""
        cp = np.ascontiguousarray(center_projected, dtype=np.float32).reshape(-1, 3)
        hd = np.ascontiguousarray(hdif, dtype=np.float32).reshape(-1)
        if len(cp) != len(hd):
            raise ValueError("one HdiF per contribution")
        ptr, rs, dev, keep = self._image(image)
        pc_n, dropped = np.zeros(self.levels, np.int32), C.c_int32()
        capi._check(_lib().eds_ct_set_ref(self._h, ptr, rs, dev, exposure, float(aff[0]), float(aff[1]), len(cp), _vp(cp), _vp(hd), _vp(pc_n),
                                          C.cast(C.byref(dropped), C.c_void_p)))
        self.pc_n = pc_n
        return pc_n, dropped.value

    def set_new(self, image, exposure=1.0):
        ptr, rs, dev, keep = self._image(image)
        capi._check(_lib().eds_ct_set_new(self._h, ptr, rs, dev, exposure))

    def track(self, T_init, aff_init=None, coarsest_lvl=None, min_res_for_abort=None):
        """trackNewestCoarse for every initial guess (count x 3 x 4, or one 3 x 4); returns RESULT records, one per try"""
        T = np.ascontiguousarray(T_init, dtype=np.float64).reshape(-1, 12)
        count = len(T)
        a = np.zeros((count, 2)) if aff_init is None else np.ascontiguousarray(aff_init, dtype=np.float64).reshape(-1, 2)
        if len(a) != count:
            raise ValueError("one affine pair per try")
        lvl = self.levels - 1 if coarsest_lvl is None else int(coarsest_lvl)
        mr = np.full(5, np.nan) if min_res_for_abort is None else np.ascontiguousarray(min_res_for_abort, dtype=np.float64)
        if mr.shape != (5,):
            raise ValueError("min_res_for_abort has 5 entries")
        out = np.zeros(count, RESULT)
        capi._check(_lib().eds_ct_track(self._h, count, _vp(T), _vp(a), lvl, _vp(mr), _vp(out)))
        return out

    def calc_res(self, lvl, T, aff=(0.0, 0.0), cutoff=None, rows=True):
        """calcRes and calcGSSSE once: dict(rs, H, b, rows)"""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(12)
        a = np.ascontiguousarray(aff, dtype=np.float64).reshape(2)
        cutoff = self.params().coarse_cutoff_th if cutoff is None else cutoff
        rs, H, b = np.zeros(6), np.zeros((8, 8)), np.zeros(8)
        r = np.zeros(int(self.pc_n[lvl]), ROW) if rows else None
        capi._check(_lib().eds_ct_calc_res(self._h, int(lvl), _vp(T), _vp(a), cutoff, _vp(rs), _vp(H), _vp(b), _vp(r)))
        return dict(rs=rs, H=H, b=b, rows=r)

    def level(self, which, lvl):
        """one level of the stored state: h x w x 3 images, h x w planes, or the pc list as n x 4 (u, v, idepth, colour)"""
        w, h = self.W >> lvl, self.H >> lvl
        shape = {REF_IMAGE: (h, w, 3), NEW_IMAGE: (h, w, 3), IDEPTH: (h, w), WEIGHT_SUMS: (h, w), PC: (h * w, 4)}[which]
        out, n = np.zeros(shape, np.float32), C.c_int32()
        capi._check(_lib().eds_ct_get_level(self._h, int(which), int(lvl), _vp(out), C.cast(C.byref(n), C.c_void_p)))
        return out[:n.value] if which == PC else out
