"""ctypes binding of include/eds_hip_undistort.h: ``dso::Undistort`` with its ``PhotometricUndistorter`` — from the camera's raw
uint8 / uint16 frame to the rectified, photometrically corrected fp32 plane the other DSO-side handles start from — on the device.

Plumbing only: K and the map are built by host code inside the C library (csrc/eds_undistort.hpp), every plane comes from the HIP
kernels behind the C ABI (csrc/eds_undistort.hip); there is no CPU fallback.  ``Undistorter`` owns one ``eds_und``.  Only
``parse_camera_text``, the reading of the four lines of DSO's camera.txt, lives here and not in the library.
"""
from __future__ import annotations

import ctypes as C
import functools
import re

import numpy as np

from . import capi

MODEL_FOV, MODEL_RADTAN, MODEL_EQUIDISTANT, MODEL_KB, MODEL_PINHOLE = range(5)
OUT_CROP, OUT_NONE, OUT_GIVEN, OUT_FULL = range(4)
U8, U16 = 0, 1
FORM_FUSED, FORM_TWO_PASS, FORM_AUTO = 0, 1, 2
MAX_SLOTS = 16


class Geometry(C.Structure):
    """``eds_und_geometry`` — what readFromFile knows after its four lines."""
    _fields_ = [("model", C.c_int32), ("pars", C.c_double * 8), ("w_org", C.c_int32), ("h_org", C.c_int32), ("out_mode", C.c_int32),
                ("out_pars", C.c_float * 5), ("w", C.c_int32), ("h", C.c_int32)]


class Settings(capi.ParamStruct):
    """``eds_und_settings`` — setting_photometricCalibration and setting_useExposure (reference src/utils/settings.cpp:117-118)."""
    _fields_ = [("photometric_calibration", C.c_int32), ("use_exposure", C.c_int32)]


@functools.lru_cache(maxsize=None)
def _lib():
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    return capi.bind(capi.UND_EXPORTS, {
        "eds_und_settings_default": ([C.POINTER(Settings)], None),
        "eds_und_create": [C.c_int, C.POINTER(Geometry), C.c_int, C.POINTER(vp)],
        "eds_und_destroy": ([vp], None),
        "eds_und_get_K": [vp, vp],
        "eds_und_get_map": [vp, vp, vp],
        "eds_und_is_passthrough": [vp, ip],
        "eds_und_set_map": [vp, vp, vp],
        "eds_und_set_photometric": [vp, vp, C.c_int, vp, C.c_int],
        "eds_und_set_settings": [vp, C.POINTER(Settings)],
        "eds_und_get_settings": [vp, C.POINTER(Settings)],
        "eds_und_set_form": [vp, C.c_int],
        "eds_und_get_form": [vp, ip],
        "eds_und_process": [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int64, C.c_int64, C.c_int, vp, C.c_float, vp],
        "eds_und_image": [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64)],
        "eds_und_get_image": [vp, C.c_int, vp],
    })


def default_settings(**over) -> Settings:
    s = Settings()
    _lib().eds_und_settings_default(C.byref(s))
    return s.update(**over)


def geometry(model, pars, w_org, h_org, out_mode, w, h, out_pars=(0, 0, 0, 0, 0)) -> Geometry:
    """``pars``: fx fy cx cy and the model's further numbers (up to 8; the rest is 0)"""
    pars, out_pars = [float(v) for v in pars], [float(v) for v in out_pars]
    if len(pars) > 8 or len(out_pars) > 5:
        raise ValueError("at most 8 parameters and 5 output parameters")
    g = Geometry(model=int(model), w_org=int(w_org), h_org=int(h_org), out_mode=int(out_mode), w=int(w), h=int(h))
    for i, v in enumerate(pars):
        g.pars[i] = v
    for i, v in enumerate(out_pars):
        g.out_pars[i] = v
    return g


_NUM = re.compile(r"[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|inf(inity)?|nan)$", re.I)
_PREFIXES = (("KannalaBrandt", MODEL_KB, 8), ("RadTan", MODEL_RADTAN, 8), ("EquiDistant", MODEL_EQUIDISTANT, 8), ("FOV", MODEL_FOV, 5),
             ("Pinhole", MODEL_PINHOLE, 5))


def _leading_numbers(tokens):
    out = []
    for t in tokens:
        if not _NUM.match(t):
            break
        out.append(float(t))
    return out


def parse_camera_text(text) -> Geometry:
    """The four lines of DSO's camera.txt as ``Undistort::getUndistorterForFile`` and ``readFromFile`` read them (reference
    src/utils/Undistort.cpp:276-362, :724-854): line 1 is 8 numbers (RadTan) or 5 (the fifth 0: Pinhole, otherwise FOV), or one of the
    prefixes KannalaBrandt / RadTan / EquiDistant (8 numbers) and FOV / Pinhole (5); line 2 the raw size; line 3 ``crop``, ``full``,
    ``none`` or five numbers; line 4 the output size.  ValueError where the reference gives up.  ``full`` parses, and
    ``eds_und_create`` refuses it."""
    lines = text.split("\n")
    lines += [""] * (4 - len(lines))
    l1, l2, l3, l4 = (s.rstrip("\r") for s in lines[:4])
    tok = l1.split()
    nums = _leading_numbers(tok)
    if len(nums) >= 8:
        model, pars = MODEL_RADTAN, nums[:8]
    elif len(nums) >= 5:
        model, pars = (MODEL_PINHOLE if np.float32(nums[4]) == 0 else MODEL_FOV), nums[:5]
    else:
        for name, model, n in _PREFIXES:
            pars = _leading_numbers(tok[1:])[:n] if tok and tok[0] == name else []
            if len(pars) == n:
                break
        else:
            raise ValueError("could not read calib file: line 1 names no camera model")

    def two_ints(line, what):
        m = re.match(r"\s*([+-]?\d+)\s+([+-]?\d+)", line)
        if not m:
            raise ValueError(f"failed to read the {what} resolution")
        return int(m.group(1)), int(m.group(2))

    w_org, h_org = two_ints(l2, "input")
    out_pars = (0, 0, 0, 0, 0)
    if l3 in ("crop", "full", "none"):
        out_mode = {"crop": OUT_CROP, "full": OUT_FULL, "none": OUT_NONE}[l3]
    else:
        out_pars = _leading_numbers(l3.split())[:5]
        if len(out_pars) != 5:
            raise ValueError("failed to read the output parameters: crop, full, none or five numbers")
        out_mode = OUT_GIVEN
    w, h = two_ints(l4, "output")
    return geometry(model, pars, w_org, h_org, out_mode, w, h, out_pars)


class _Plane:
    """the base of a ``capi.DeviceView`` over a slot: keeps the undistorter, and so the plane, alive"""

    def __init__(self, owner, ptr):
        self.owner, self.ptr, self.dtype = owner, int(ptr), np.dtype(np.float32)


_vp = capi.vp
_RAW_TYPES = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16}


class Undistorter(capi.OwnedHandle):
    """The undistorter of one camera: K, the map, the photometric tables and ``slots`` output planes in device memory."""
    _destroy = "eds_und_destroy"

    def __init__(self, geometry, slots=1, device=0):
        self._h = C.c_void_p()
        if not isinstance(geometry, Geometry):
            raise TypeError("geometry: an undistort.Geometry (undistort.geometry(...) or parse_camera_text(...))")
        self.geometry, self.slots, self.device = geometry, int(slots), int(device)
        self.w, self.h, self.w_org, self.h_org = geometry.w, geometry.h, geometry.w_org, geometry.h_org
        capi._check(_lib().eds_und_create(self.device, C.byref(geometry), self.slots, C.byref(self._h)))

    @property
    def K(self):
        out = np.zeros((3, 3), np.float64)
        capi._check(_lib().eds_und_get_K(self._h, _vp(out)))
        return out

    @property
    def map(self):
        """(remapX, remapY), h x w floats each: (-1, -1) or a position inside the raw image"""
        mx, my = np.zeros((self.h, self.w), np.float32), np.zeros((self.h, self.w), np.float32)
        capi._check(_lib().eds_und_get_map(self._h, _vp(mx), _vp(my)))
        return mx, my

    @property
    def passthrough(self):
        v = C.c_int()
        capi._check(_lib().eds_und_is_passthrough(self._h, C.byref(v)))
        return bool(v.value)

    def set_map(self, mapx, mapy):
        mx, my = (np.ascontiguousarray(m, dtype=np.float32) for m in (mapx, mapy))
        if mx.shape != (self.h, self.w) or my.shape != (self.h, self.w):
            raise ValueError(f"the maps must be {self.h} x {self.w}")
        capi._check(_lib().eds_und_set_map(self._h, _vp(mx), _vp(my)))

    def set_photometric(self, G, vignette):
        """G: 256 .. 65 536 strictly increasing floats; vignette: h_org x w_org, uint8 or uint16"""
        g = np.ascontiguousarray(G, dtype=np.float32).reshape(-1)
        v = np.ascontiguousarray(vignette)
        if v.dtype not in _RAW_TYPES or v.shape != (self.h_org, self.w_org):
            raise ValueError(f"the vignette must be uint8 or uint16, {self.h_org} x {self.w_org}")
        capi._check(_lib().eds_und_set_photometric(self._h, _vp(g), g.size, _vp(v), _RAW_TYPES[v.dtype]))

    def settings(self) -> Settings:
        s = Settings()
        capi._check(_lib().eds_und_get_settings(self._h, C.byref(s)))
        return s

    def set_settings(self, **over):
        s = self.settings().update(**over)
        capi._check(_lib().eds_und_set_settings(self._h, C.byref(s)))

    @property
    def form(self):
        v = C.c_int()
        capi._check(_lib().eds_und_get_form(self._h, C.byref(v)))
        return v.value

    @form.setter
    def form(self, v):
        capi._check(_lib().eds_und_set_form(self._h, int(v)))

    def process(self, raw, exposures, factor=1.0, first_slot=0):
        """``raw``: count x h_org x w_org (or h_org x w_org: one frame) of uint8 or uint16 — a numpy array, whose row and frame strides
        are kept, or device memory (``__cuda_array_interface__``, a ``(ptr, shape, strides, dtype)`` tuple).  ``exposures``: one per
        frame.  Fills slots first_slot .. ; returns the frames' exposure times (1 when use_exposure is off)."""
        on_device = capi.is_device_source(raw)
        if on_device:
            ptr, shape, est, dt = capi.device_array_info(raw)
        else:
            a = np.asarray(raw)
            if a.dtype not in _RAW_TYPES:
                raise ValueError(f"raw frames are uint8 or uint16, not {a.dtype}")
            it = a.dtype.itemsize
            ok = a.ndim in (2, 3) and a.strides[-1] == it and all(s % it == 0 and s > 0 for s in a.strides)
            if not ok or a.strides[-2] < it * a.shape[-1] or (a.ndim == 3 and a.shape[0] > 1 and a.strides[0] < a.strides[1] * (a.shape[1] - 1) + it * a.shape[2]):
                a = np.ascontiguousarray(a)
            ptr, shape, est, dt = a.ctypes.data, a.shape, tuple(s // it for s in a.strides), a.dtype
        if dt not in _RAW_TYPES:
            raise ValueError(f"raw frames are uint8 or uint16, not {dt}")
        if len(shape) == 2:
            shape, est = (1,) + tuple(shape), (0,) + tuple(est)
        if len(shape) != 3 or tuple(shape[1:]) != (self.h_org, self.w_org) or shape[0] < 1 or est[2] != 1:
            raise ValueError(f"raw frames must be count x {self.h_org} x {self.w_org} with contiguous rows, not {tuple(shape)}")
        count = int(shape[0])
        e = np.ascontiguousarray(np.asarray(exposures, dtype=np.float32).reshape(-1))
        if e.size != count:
            raise ValueError(f"{count} frames and {e.size} exposures")
        out = np.zeros(count, np.float32)
        capi._check(_lib().eds_und_process(self._h, int(first_slot), count, C.c_void_p(ptr), _RAW_TYPES[np.dtype(dt)], int(est[1]),
                                           int(est[0]) if count > 1 else 0, 1 if on_device else 0, _vp(e), float(factor), _vp(out)))
        return out

    def image(self, slot):
        """the device plane of a slot, h x w floats, as a ``capi.DeviceView``: what ``Selector.set_image``, ``CoarseTracker.set_new``
        and the other mirrors' setters accept as device memory.  Holds what the last ``process`` wrote there."""
        p, rs = C.c_void_p(), C.c_int64()
        capi._check(_lib().eds_und_image(self._h, int(slot), C.byref(p), C.byref(rs)))
        return capi.DeviceView(_Plane(self, p.value), (self.h, self.w), (4 * rs.value, 4), 0)

    def get_image(self, slot):
        out = np.zeros((self.h, self.w), np.float32)
        capi._check(_lib().eds_und_get_image(self._h, int(slot), _vp(out)))
        return out
