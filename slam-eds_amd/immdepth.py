"""ctypes binding of include/eds_hip_immdepth.h: a keyframe's immature points seeded from a depth map that lives on the device — the
map's k-d tree, the nearest-neighbour walk per selected pixel and ``ImmaturePoint``'s second constructor, without a per-point or
per-pixel array crossing the bus.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_immdepth.hip); there is no CPU fallback.
``ImmatureDepth`` wraps an ``immature.ImmaturePoints``, whose ``eds_imm`` owns the state; the points it creates are ordinary points of
that object.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi

WALK_GLOBAL = 1


class Info(C.Structure):
    """``eds_imd_info``"""
    _fields_ = [("map_set", C.c_int32), ("map_n", C.c_int32), ("tree_on_host", C.c_int32), ("waits", C.c_int32), ("walk", C.c_int32),
                ("reserved", C.c_int32), ("nn_kernel_ms", C.c_float), ("queue_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


@functools.lru_cache(maxsize=None)
def _lib():
    vp, i = C.c_void_p, C.c_int
    return capi.bind(capi.IMD_EXPORTS, {
        "eds_imd_set_depth_map": [vp, i, vp, vp, i, C.POINTER(i)],
        "eds_imd_create_points_selected": [vp, i, vp, i, i, i, i, vp, vp, C.POINTER(i), vp],
        "eds_imd_create_points": [vp, i, i, vp, vp, i, vp, vp, vp],
        "eds_imd_get_nearest": [vp, i, vp, vp, vp],
        "eds_imd_get_tree": [vp, vp, vp, vp],
        "eds_imd_set_debug": [vp, i],
        "eds_imd_get_info": [vp, C.POINTER(Info)],
    })


def _scale(scale):
    return None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(2)


def _device_vector(obj, dtype, width, name):
    """(ptr, n) of a dense device array n [x width] of `dtype`"""
    ptr, shape, est, dt = capi.device_array_info(obj)
    while len(shape) > (1 if width == 1 else 2) and shape[0] == 1:      # one map of a count x stride [x 2] result
        shape, est = shape[1:], est[1:]
    want = (1,) if width == 1 else (width, 1)
    if dt != np.dtype(dtype) or len(shape) != len(want) or (width > 1 and shape[1] != width) or tuple(est) != want:
        raise ValueError(f"{name} must be a dense device array n" + (f" x {width}" if width > 1 else "") + f" of {np.dtype(dtype).name}, not {shape} {dt.name}")
    return ptr, int(shape[0])


class ImmatureDepth:
    """Depth-seeded creation of the points of ``immature_points`` (an ``immature.ImmaturePoints``)."""

    def __init__(self, immature_points):
        self.imm = immature_points
        _lib()

    @property
    def _h(self):
        return self.imm._h

    def set_depth_map(self, xy, idp, n=None):
        """The map the next create calls seed from: numpy arrays (n x 2 and n doubles) or device memory (anything with
        ``__cuda_array_interface__``; `n`: the leading points that count, as ``map.window_depth_maps`` reports them).  Returns True
        where the host built the tree (an ambiguous map, or one beyond ``capi.tree_capacity()``)."""
        on_host = C.c_int()
        if capi.is_device_source(xy) or capi.is_device_source(idp):
            pxy, nxy = _device_vector(xy, np.float64, 2, "xy")
            pidp, nidp = _device_vector(idp, np.float64, 1, "idp")
            n = min(nxy, nidp) if n is None else int(n)
            if n > min(nxy, nidp):
                raise ValueError(f"n = {n} is more than the arrays hold")
            capi._check(_lib().eds_imd_set_depth_map(self._h, n, C.c_void_p(pxy or None), C.c_void_p(pidp or None), 1, C.byref(on_host)))
        else:
            a = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
            b = np.ascontiguousarray(idp, dtype=np.float64).reshape(-1)
            n = len(a) if n is None else int(n)
            if n > len(a) or n > len(b):
                raise ValueError(f"n = {n} is more than the arrays hold")
            capi._check(_lib().eds_imd_set_depth_map(self._h, n, capi.vp(a), capi.vp(b), 0, C.byref(on_host)))
        return bool(on_host.value)

    def create_points_selected(self, host, selector, rect=None, scale=None):
        """The loop of the header for the pixels ``selector`` chose inside the inclusive rectangle (None: DSO's own bounds,
        3 .. W - 5 and 3 .. H - 5).  Returns (alive mask, (GOOD, UNINITIALIZED) among the alive)."""
        imm = self.imm
        x0, y0, x1, y1 = (3, 3, imm.W - 5, imm.H - 5) if rect is None else (int(v) for v in rect)
        alive = np.zeros(max(1, imm.max_points), dtype=np.uint8)
        n, counts, s = C.c_int(), np.zeros(2, np.int32), _scale(scale)
        capi._check(_lib().eds_imd_create_points_selected(self._h, int(host), selector._h, x0, y0, x1, y1, capi.vp(s), capi.vp(alive), C.byref(n),
                                                          capi.vp(counts)))
        return alive[:n.value].astype(bool), (int(counts[0]), int(counts[1]))

    def create_points(self, host, uv, type=None, scale=None):
        """The same for a caller's own pixels: numpy (n x 2 int32, n floats) or both in device memory."""
        counts, s = np.zeros(2, np.int32), _scale(scale)
        if capi.is_device_source(uv):
            puv, n = _device_vector(uv, np.int32, 2, "uv")
            ptyp, nt = _device_vector(type, np.float32, 1, "type")
            if nt != n:
                raise ValueError("type: one float per point")
            alive = np.zeros(max(n, 1), dtype=np.uint8)
            capi._check(_lib().eds_imd_create_points(self._h, int(host), n, C.c_void_p(puv or None), C.c_void_p(ptyp or None), 1, capi.vp(s), capi.vp(alive),
                                                     capi.vp(counts)))
        else:
            a = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
            n = len(a)
            typ = np.ascontiguousarray(np.ones(n) if type is None else type, dtype=np.float32)
            if typ.shape != (n,):
                raise ValueError("type: one float per point")
            alive = np.zeros(max(n, 1), dtype=np.uint8)
            capi._check(_lib().eds_imd_create_points(self._h, int(host), n, capi.vp(a), capi.vp(typ), 0, capi.vp(s), capi.vp(alive), capi.vp(counts)))
        return alive[:n].astype(bool), (int(counts[0]), int(counts[1]))

    def nearest(self, host):
        """what each point of the last create call on `host` took from the map: dict(index, idepth, distance)"""
        n = self.imm.num_points(host)
        o = dict(index=np.zeros(n, np.int32), idepth=np.zeros(n, np.float32), distance=np.zeros(n, np.float64))
        capi._check(_lib().eds_imd_get_nearest(self._h, int(host), *[capi.vp(v) for v in o.values()]))
        return o

    def tree(self):
        """the map in tree order: dict(perm, txy, tidp)"""
        n = self.info()["map_n"]
        o = dict(perm=np.zeros(n, np.int32), txy=np.zeros((n, 2), np.float64), tidp=np.zeros(n, np.float64))
        capi._check(_lib().eds_imd_get_tree(self._h, *[capi.vp(v) for v in o.values()]))
        return o

    def set_debug(self, timing=False):
        """for measurements: whether the next create calls time their kernels with events"""
        capi._check(_lib().eds_imd_set_debug(self._h, 1 if timing else 0))

    def info(self):
        i = Info()
        capi._check(_lib().eds_imd_get_info(self._h, C.byref(i)))
        return i.as_dict()
