"""ctypes binding of include/eds_hip_select.h: DSO's pixel selector — ``PixelSelector::makeMaps`` with ``makeHists`` and ``select`` over
levels 0 .. 2 of ``makeImages`` including ``absSquaredGrad`` — on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_pixsel.hip); there is no CPU fallback.  ``Selector``
owns one ``eds_sel``.  The random table is an input: ``reference_pattern`` is what the reference's constructor draws.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi

THS, THS_SMOOTHED = 0, 1
MAX_POTENTIAL = 1 << 30


class Params(capi.ParamStruct):
    """``eds_sel_params`` — the setting_* values the selector reads (reference src/utils/settings.cpp:145-148)."""
    _fields_ = [("min_grad_hist_cut", C.c_float), ("min_grad_hist_add", C.c_float), ("grad_downweight_per_level", C.c_float),
                ("select_direction_distribution", C.c_int32)]


class Pass(C.Structure):
    """``eds_sel_pass`` — one select pass of ``make_maps``."""
    _fields_ = [("potential", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32), ("n4", C.c_int32)]


@functools.lru_cache(maxsize=None)
def _lib():
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    return capi.bind(capi.SEL_EXPORTS, {
        "eds_sel_params_default": ([C.POINTER(Params)], None),
        "eds_sel_create": [C.c_int] * 3 + [C.POINTER(vp)],
        "eds_sel_destroy": ([vp], None),
        "eds_sel_set_params": [vp, C.POINTER(Params)],
        "eds_sel_get_params": [vp, C.POINTER(Params)],
        "eds_sel_set_random_pattern": [vp, vp, C.c_size_t],
        "eds_sel_fill_reference_pattern": [vp, C.c_size_t],
        "eds_sel_set_potential": [vp, C.c_int],
        "eds_sel_get_potential": [vp, ip],
        "eds_sel_set_image": [vp, vp, C.c_int64, C.c_int, vp],
        "eds_sel_make_maps": [vp, C.c_float, C.c_int, C.c_float, ip, C.POINTER(Pass), C.c_int, ip, vp],
        "eds_sel_get_map": [vp, vp],
        "eds_sel_get_selection": [vp, ip, vp, vp],
        "eds_sel_get_level": [vp, C.c_int, vp],
        "eds_sel_get_thresholds": [vp, C.c_int, vp],
        "eds_sel_get_scan_info": [vp, ip, ip],
    })


def default_params(**over) -> Params:
    p = Params()
    _lib().eds_sel_params_default(C.byref(p))
    return p.update(**over)


def reference_pattern(n):
    """The ``randomPattern`` of the reference's constructor: srand(3141592), then n times rand() & 0xFF.  Reseeds the C library's generator."""
    out = np.zeros(int(n), np.uint8)
    capi._check(_lib().eds_sel_fill_reference_pattern(out.ctypes.data_as(C.c_void_p), out.size))
    return out


_vp = capi.vp


class Selector(capi.OwnedHandle):
    """The pixel selector of one image size, in device memory.  ``potential`` is the reference's currentPotential."""
    _destroy = "eds_sel_destroy"

    def __init__(self, H, W, device=0, table=None, **params):
        self._h = C.c_void_p()
        self.H, self.W, self.device = int(H), int(W), int(device)
        capi._check(_lib().eds_sel_create(self.device, self.H, self.W, C.byref(self._h)))
        self.passes = []
        self.pass_maps = None
        if params:
            self.set_params(**params)
        if table is not None:
            self.set_random_pattern(table)

    def set_params(self, **over):
        p = self.params().update(**over)
        capi._check(_lib().eds_sel_set_params(self._h, C.byref(p)))

    def params(self) -> Params:
        p = Params()
        capi._check(_lib().eds_sel_get_params(self._h, C.byref(p)))
        return p

    def set_random_pattern(self, table):
        t = np.ascontiguousarray(table, dtype=np.uint8).reshape(-1)
        capi._check(_lib().eds_sel_set_random_pattern(self._h, _vp(t), t.size))

    @property
    def potential(self):
        v = C.c_int()
        capi._check(_lib().eds_sel_get_potential(self._h, C.byref(v)))
        return v.value

    @potential.setter
    def potential(self, v):
        capi._check(_lib().eds_sel_set_potential(self._h, int(v)))

    def set_image(self, image, B=None):
        """fp32 intensities 0 .. 255: a numpy array H x W (its row stride is kept) or device memory (``capi.DeviceArray`` and the like);
        B: None, or the 256 floats of ``CalibHessian::B``"""
        b = None if B is None else np.ascontiguousarray(B, dtype=np.float32).reshape(256)
        if not capi.is_device_source(image):
            a = np.asarray(image, dtype=np.float32)
            if a.shape != (self.H, self.W):
                raise ValueError(f"the image must be {self.H} x {self.W}, not {a.shape}")
            if a.strides[1] != 4 or a.strides[0] % 4 or a.strides[0] < 4 * self.W:
                a = np.ascontiguousarray(a)
            capi._check(_lib().eds_sel_set_image(self._h, _vp(a), a.strides[0] // 4, 0, _vp(b)))
            return
        ptr, shape, est, dt = capi.device_array_info(image)
        if dt != np.float32 or tuple(shape) != (self.H, self.W) or est[1] != 1:
            raise ValueError(f"a device image must be float32 {self.H} x {self.W} with contiguous rows")
        capi._check(_lib().eds_sel_set_image(self._h, C.c_void_p(ptr), int(est[0]), 1, _vp(b)))

    def make_maps(self, density, recursions_left=1, th_factor=1.0, keep_pass_maps=False):
        """``makeMaps``; returns numHaveSub.  ``passes`` then holds (potential, n2, n3, n4) of every select pass, ``pass_maps`` the map
        after each of them when asked for."""
        cap = int(recursions_left) + 1
        ps = (Pass * max(1, cap))()
        n, npass = C.c_int(), C.c_int()
        maps = np.zeros((max(1, cap), self.H, self.W), np.uint8) if keep_pass_maps else None
        capi._check(_lib().eds_sel_make_maps(self._h, float(density), int(recursions_left), float(th_factor), C.byref(n), ps, max(1, cap),
                                             C.byref(npass), _vp(maps)))
        self.passes = [(p.potential, p.n2, p.n3, p.n4) for p in ps[:npass.value]]
        self.pass_maps = None if maps is None else maps[:npass.value]
        return n.value

    def map(self):
        out = np.zeros((self.H, self.W), np.uint8)
        capi._check(_lib().eds_sel_get_map(self._h, _vp(out)))
        return out

    @property
    def num_selected(self):
        n = C.c_int()
        capi._check(_lib().eds_sel_get_selection(self._h, C.byref(n), None, None))
        return n.value

    def selection(self):
        """uv (n x 2 int32) and type (n floats) of the map's non-zero pixels in row-major order"""
        n = self.num_selected
        uv, typ = np.zeros((n, 2), np.int32), np.zeros(n, np.float32)
        m = C.c_int()
        capi._check(_lib().eds_sel_get_selection(self._h, C.byref(m), _vp(uv), _vp(typ)))
        return uv, typ

    def level(self, lvl):
        """(H >> lvl) x (W >> lvl) x (colour, dx, dy, absSquaredGrad)"""
        out = np.zeros((self.H >> lvl, self.W >> lvl, 4), np.float32)
        capi._check(_lib().eds_sel_get_level(self._h, int(lvl), _vp(out)))
        return out

    def thresholds(self, which=THS_SMOOTHED):
        out = np.zeros((self.H // 32, self.W // 32), np.float32)
        capi._check(_lib().eds_sel_get_thresholds(self._h, int(which), _vp(out)))
        return out

    def scan_info(self):
        """(ambiguous cells, n2 of the certain cells alone) of the last select pass"""
        a, c = C.c_int(), C.c_int()
        capi._check(_lib().eds_sel_get_scan_info(self._h, C.byref(a), C.byref(c)))
        return a.value, c.value
