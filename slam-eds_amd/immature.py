"""ctypes binding of include/eds_hip_immature.h: DSO's immature points as EDS uses them on its mapping side — makeImages level 0, both
``ImmaturePoint`` constructors and ``ImmaturePoint::traceOn`` for every point of a range of host frames, on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_immature.hip); there is no CPU fallback.
``ImmaturePoints`` owns one ``eds_imm``; its accessors carry the reference's member names.  ``precalc`` forms the three arguments of
``traceOn`` the way DSO's ``traceNewCoarse`` does.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi

GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)      # dso::ImmaturePointStatus
STATUS_NAMES = ("IPS_GOOD", "IPS_OOB", "IPS_OUTLIER", "IPS_SKIPPED", "IPS_BADCONDITION", "IPS_UNINITIALIZED")
HOST_IMAGE, TARGET_IMAGE = 0, 1


class Params(capi.ParamStruct):
    """``eds_imm_params`` — the setting_* values the constructors and traceOn read (reference src/utils/settings.cpp:90-165)."""
    _fields_ = [("max_pix_search", C.c_float), ("trace_stepsize", C.c_float), ("trace_gn_iterations", C.c_int32),
                ("trace_gn_threshold", C.c_float), ("trace_extra_slack_on_th", C.c_float), ("trace_slack_interval", C.c_float),
                ("trace_min_improvement_factor", C.c_float), ("min_trace_test_radius", C.c_int32), ("huber_th", C.c_float),
                ("outlier_th", C.c_float), ("outlier_th_sum_component", C.c_float), ("overall_energy_th_weight", C.c_float)]


@functools.lru_cache(maxsize=None)
def _lib():
    vp, i64 = C.c_void_p, C.c_int64
    return capi.bind(capi.IMM_EXPORTS, {
        "eds_imm_params_default": ([C.POINTER(Params)], None),
        "eds_imm_create": [C.c_int] * 6 + [C.POINTER(vp)],
        "eds_imm_destroy": ([vp], None),
        "eds_imm_set_params": [vp, C.POINTER(Params)],
        "eds_imm_get_params": [vp, C.POINTER(Params)],
        "eds_imm_set_host_images": [vp, C.c_int, C.c_int, vp, i64, i64, C.c_int],
        "eds_imm_set_target_images": [vp, C.c_int, C.c_int, vp, i64, i64, C.c_int],
        "eds_imm_create_points": [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp],
        "eds_imm_create_points_selected": [vp, C.c_int, vp] + [C.c_int] * 4 + [vp, C.POINTER(C.c_int)],
        "eds_imm_num_points": [vp, C.c_int, C.POINTER(C.c_int)],
        "eds_imm_trace": [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp],
        "eds_imm_get": [vp, C.c_int] + [vp] * 6,
        "eds_imm_get_points": [vp, C.c_int] + [vp] * 5,
        "eds_imm_get_image": [vp, C.c_int, C.c_int, vp],
    })


def default_params(**over) -> Params:
    p = Params()
    _lib().eds_imm_params_default(C.byref(p))
    return p.update(**over)


def precalc(K, R, t, aff_host=(0.0, 0.0), aff_target=(0.0, 0.0), exposures=(1.0, 1.0)):
    """``hostToFrame_KRKi``, ``hostToFrame_Kt``, ``hostToFrame_affine`` as traceNewCoarse forms them: K (3 x 3 or fx, fy, cx, cy), the
    rotation and translation of hostToNew narrowed to fp32, the products in fp32; the affine pair is AffLight::fromToVecExposure
    (exposure_host, exposure_target, (a, b) of host and target) in fp64, narrowed."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (4,):
        K = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    K32 = K.astype(np.float32)
    Ki32 = np.linalg.inv(K).astype(np.float32)
    KRKi = (K32 @ np.asarray(R, dtype=np.float64).astype(np.float32)) @ Ki32
    Kt = K32 @ np.asarray(t, dtype=np.float64).astype(np.float32)
    eh, et = (float(x) for x in exposures)
    if eh == 0 or et == 0:
        eh = et = 1.0
    a = np.exp(float(aff_target[0]) - float(aff_host[0])) * et / eh
    b = float(aff_target[1]) - a * float(aff_host[1])
    return KRKi.astype(np.float32), Kt.astype(np.float32), np.array([a, b], dtype=np.float32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class ImmaturePoints(capi.OwnedHandle):
    """The immature points of up to ``max_hosts`` host frames and the frames they are traced on, in device memory."""
    _destroy = "eds_imm_destroy"

    def __init__(self, H, W, max_hosts=1, max_points_per_host=2000, max_targets=1, device=0, **params):
        self._h = C.c_void_p()
        self.H, self.W, self.max_hosts, self.max_points, self.max_targets, self.device = int(H), int(W), int(max_hosts), int(max_points_per_host), int(max_targets), int(device)
        capi._check(_lib().eds_imm_create(self.device, self.H, self.W, self.max_hosts, self.max_points, self.max_targets, C.byref(self._h)))
        if params:
            self.set_params(**params)

    def set_params(self, **over):
        p = self.params().update(**over)
        capi._check(_lib().eds_imm_set_params(self._h, C.byref(p)))

    def params(self) -> Params:
        p = Params()
        capi._check(_lib().eds_imm_get_params(self._h, C.byref(p)))
        return p

    def _set_images(self, fn, first, images):
        if not capi.is_device_source(images):
            a = _f32(images)
            a = a[None] if a.ndim == 2 else a
            if a.shape[1:] != (self.H, self.W):
                raise ValueError(f"images must be count x {self.H} x {self.W}, not {a.shape}")
            capi._check(fn(self._h, int(first), a.shape[0], a.ctypes.data_as(C.c_void_p), 0, 0, 0))
            return
        ptr, shape, est, dt = capi.device_array_info(images)        # device memory: __cuda_array_interface__ or (ptr, shape, strides, dtype)
        if len(shape) == 2:
            shape, est = (1,) + tuple(shape), (0,) + tuple(est)
        if dt != np.float32 or len(shape) != 3 or tuple(shape[1:]) != (self.H, self.W) or est[2] != 1:
            raise ValueError(f"device images must be float32 count x {self.H} x {self.W} with contiguous rows")
        capi._check(fn(self._h, int(first), int(shape[0]), C.c_void_p(ptr), int(est[0]) if shape[0] > 1 else 0, int(est[1]), 1))

    def set_host_images(self, first, images):
        """fp32 intensities 0 .. 255: a numpy array (count x H x W or H x W) or device memory (``capi.DeviceArray`` and the like)"""
        self._set_images(_lib().eds_imm_set_host_images, first, images)

    def set_target_images(self, first, images):
        self._set_images(_lib().eds_imm_set_target_images, first, images)

    def create_points(self, host, uv, type=None, idepth=None, distance=None):
        """Both constructors for the points of ``host``; returns the alive mask (False: the pattern left the image)."""
        uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
        n = len(uv)
        typ = _f32(np.ones(n) if type is None else type)
        if typ.shape != (n,):
            raise ValueError("type: one float per point")
        idp = None if idepth is None else _f32(idepth)
        dist = None if distance is None else np.ascontiguousarray(distance, dtype=np.float64)
        if (idp is not None and idp.shape != (n,)) or (dist is not None and dist.shape != (n,)):
            raise ValueError("idepth and distance: one value per point")
        alive = np.zeros(n, dtype=np.uint8)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        capi._check(_lib().eds_imm_create_points(self._h, int(host), n, vp(uv), vp(typ), vp(idp), vp(dist), vp(alive)))
        return alive.astype(bool)

    def create_points_selected(self, host, selector, rect=None):
        """The first constructor for the pixels ``selector`` (a ``select.Selector`` after ``make_maps``) chose inside the inclusive
        rectangle ``(x_min, y_min, x_max, y_max)``, read from the device; ``None`` is DSO's own bounds, 3 .. W - 5 and 3 .. H - 5.
        Returns the alive mask, one entry per point created."""
        x0, y0, x1, y1 = (3, 3, self.W - 5, self.H - 5) if rect is None else (int(v) for v in rect)
        alive = np.zeros(max(1, min(selector.num_selected, self.max_points)), dtype=np.uint8)
        n = C.c_int()
        capi._check(_lib().eds_imm_create_points_selected(self._h, int(host), selector._h, x0, y0, x1, y1, alive.ctypes.data_as(C.c_void_p), C.byref(n)))
        return alive[:n.value].astype(bool)

    def num_points(self, host):
        n = C.c_int()
        capi._check(_lib().eds_imm_num_points(self._h, int(host), C.byref(n)))
        return n.value

    def trace(self, first_host, target_index, KRKi, Kt, aff):
        """traceOn for hosts first_host .. first_host + count - 1; returns count x 6 status counts (GOOD .. UNINITIALIZED)."""
        ti = np.ascontiguousarray(np.atleast_1d(target_index), dtype=np.int32)
        count = len(ti)
        k, t, a = _f32(KRKi).reshape(-1, 9), _f32(Kt).reshape(-1, 3), _f32(aff).reshape(-1, 2)
        if not (len(k) == len(t) == len(a) == count):
            raise ValueError("one KRKi, Kt and affine pair per host")
        out = np.zeros((count, 6), dtype=np.int32)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        capi._check(_lib().eds_imm_trace(self._h, int(first_host), count, vp(ti), vp(k), vp(t), vp(a), vp(out)))
        return out

    def get(self, host):
        """idepth_min, idepth_max, quality, lastTraceStatus, lastTraceUV, lastTracePixelInterval per point"""
        n = self.num_points(host)
        o = dict(idepth_min=np.zeros(n, np.float32), idepth_max=np.zeros(n, np.float32), quality=np.zeros(n, np.float32),
                 lastTraceStatus=np.zeros(n, np.int32), lastTraceUV=np.zeros((n, 2), np.float32), lastTracePixelInterval=np.zeros(n, np.float32))
        capi._check(_lib().eds_imm_get(self._h, int(host), *[v.ctypes.data_as(C.c_void_p) for v in o.values()]))
        return o

    def points(self, host):
        """color, weights, gradH (n x 2 x 2), energyTH and the alive mask, as the constructor left them"""
        n = self.num_points(host)
        o = dict(color=np.zeros((n, 8), np.float32), weights=np.zeros((n, 8), np.float32), gradH=np.zeros((n, 2, 2), np.float32),
                 energyTH=np.zeros(n, np.float32), alive=np.zeros(n, np.uint8))
        capi._check(_lib().eds_imm_get_points(self._h, int(host), *[v.ctypes.data_as(C.c_void_p) for v in o.values()]))
        o["alive"] = o["alive"].astype(bool)
        return o

    def image(self, which, index):
        """the stored frame, H x W x (colour, dx, dy)"""
        out = np.zeros((self.H, self.W, 3), np.float32)
        capi._check(_lib().eds_imm_get_image(self._h, int(which), int(index), out.ctypes.data_as(C.c_void_p)))
        return out
