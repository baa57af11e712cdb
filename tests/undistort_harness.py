"""ctypes side of tests/host_logic/undistort_harness.cpp: csrc/eds_undistort.hpp (namespace edsund — the set-up the library runs on the
host, and the per-pixel functions its kernels call) compiled with g++ into a temporary directory where the tests run.
``HostUndistorter`` has the interface of ``undistort.Undistorter`` (one slot, host frames), so one comparison serves the host
restatement and the device."""
import ctypes as C
import importlib
import os

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "undistort_harness.cpp")
RC_OK, RC_INVALID, RC_NOT_USABLE = 0, -1, -3
_vp = C.c_void_p
_p = hb.p
_lib = None


def _und():
    return importlib.import_module("slam-eds_amd.undistort")


def load_harness():
    global _lib
    if _lib is None:
        _lib = hb.load_library("undistort", SRC)
        _lib.und_new.restype = _vp
        _lib.und_new.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.und_free.argtypes = [_vp]
        _lib.und_free.restype = None
        for n in ("und_get_K", "und_get_pars", "und_settings_default"):
            getattr(_lib, n).argtypes = [_vp] * (1 if n == "und_settings_default" else 2)
            getattr(_lib, n).restype = None
        _lib.und_get_map.argtypes = [_vp, _vp, _vp]
        _lib.und_get_map.restype = None
        _lib.und_info.argtypes = [_vp, _vp, _vp]
        _lib.und_info.restype = None
        _lib.und_set_map.argtypes = [_vp, _vp, _vp]
        _lib.und_set_photometric.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int]
        _lib.und_set_settings.argtypes = [_vp, _vp]
        _lib.und_get_photometric.argtypes = [_vp, _vp, _vp]
        _lib.und_process.argtypes = [_vp, _vp, C.c_int, C.c_int64, C.c_float, C.c_float, _vp, _vp]
        u = _und()
        assert _lib.und_geometry_size() == C.sizeof(u.Geometry) == 112 and _lib.und_settings_size() == C.sizeof(u.Settings) == 8
    return _lib


class HostError(Exception):
    def __init__(self, code, iterations=0):
        super().__init__(f"edsund rc {code}")
        self.code, self.iterations = code, iterations


class HostUndistorter:
    """edsund::setup, set_photometric and process_host behind the interface of slam-eds_amd.undistort.Undistorter"""

    def __init__(self, geometry, slots=1, device=0):
        self.hl = load_harness()
        rc, it = C.c_int(), C.c_int()
        self._h = _vp(self.hl.und_new(C.addressof(geometry), C.byref(rc), C.byref(it)))
        if not self._h:
            raise HostError(rc.value, it.value)
        self.w, self.h, self.w_org, self.h_org = geometry.w, geometry.h, geometry.w_org, geometry.h_org
        self._st = dict(photometric_calibration=2, use_exposure=1)
        self._plane = np.zeros((self.h, self.w), np.float32)

    def close(self):
        if getattr(self, "_h", None):
            self.hl.und_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def K(self):
        out = np.zeros((3, 3))
        self.hl.und_get_K(self._h, _p(out))
        return out

    @property
    def pars(self):
        out = np.zeros(8)
        self.hl.und_get_pars(self._h, _p(out))
        return out

    @property
    def map(self):
        mx, my = np.zeros((self.h, self.w), np.float32), np.zeros((self.h, self.w), np.float32)
        self.hl.und_get_map(self._h, _p(mx), _p(my))
        return mx, my

    def info(self):
        out, rng = np.zeros(8, np.int64), np.zeros(4, np.float32)
        self.hl.und_info(self._h, _p(out), _p(rng))
        return dict(passthrough=bool(out[0]), relative=bool(out[1]), iterations=int(out[2]), shrinks=tuple(int(v) for v in out[3:7]),
                    rule_pixels=int(out[7]), range=tuple(rng))

    @property
    def passthrough(self):
        return self.info()["passthrough"]

    def set_map(self, mapx, mapy):
        mx, my = (np.ascontiguousarray(m, np.float32) for m in (mapx, mapy))
        rc = self.hl.und_set_map(self._h, _p(mx), _p(my))
        if rc:
            raise HostError(rc)

    def set_photometric(self, G, vignette):
        g, v = np.ascontiguousarray(G, np.float32).reshape(-1), np.ascontiguousarray(vignette)
        rc = self.hl.und_set_photometric(self._h, _p(g), g.size, _p(v), 1 if v.dtype == np.uint16 else 0)
        if rc:
            raise HostError(rc)

    def photometric(self):
        """(G, vignetteMapInv), or None without a calibration"""
        d = self.hl.und_get_photometric(self._h, None, None)
        if not d:
            return None
        G, vinv = np.zeros(d, np.float32), np.zeros((self.h_org, self.w_org), np.float32)
        self.hl.und_get_photometric(self._h, _p(G), _p(vinv))
        return G, vinv

    def set_settings(self, **over):
        self._st.update(over)
        s = np.array([self._st["photometric_calibration"], self._st["use_exposure"]], np.int32)
        rc = self.hl.und_set_settings(self._h, _p(s))
        if rc:
            raise HostError(rc)

    def process(self, raw, exposures, factor=1.0, first_slot=0):
        a = np.asarray(raw)
        if a.ndim == 2:
            a = a[None]
        e = np.asarray(exposures, np.float32).reshape(-1)
        out = np.zeros(len(a), np.float32)
        self.planes = np.zeros((len(a), self.h, self.w), np.float32)
        for k, frame in enumerate(a):
            f = np.ascontiguousarray(frame)
            eo = C.c_float()
            rc = self.hl.und_process(self._h, _p(f), 1 if f.dtype == np.uint16 else 0, 0, C.c_float(e[k]), C.c_float(factor), _p(self.planes[k]), C.byref(eo))
            if rc:
                raise HostError(rc)
            out[k] = eo.value
        return out

    def get_image(self, slot):
        return self.planes[slot].copy()
