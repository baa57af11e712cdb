"""ctypes binding of include/eds_hip_init.h: DSO's two-frame initialiser (``dso::CoarseInitializer``) — the first frame's pyramid and
points, and the whole of ``trackFrame`` in one kernel launch per new frame — on the device.

Plumbing only: every number comes from the HIP kernels behind the C ABI (csrc/eds_init.hip); there is no CPU fallback.
``CoarseInitializer`` owns one ``eds_ini`` and keeps the reference's member names (``setFirst``, ``trackFrame``, ``rescale``).  Images
and status maps may be numpy arrays or anything with ``__cuda_array_interface__``.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import capi

MAX_LEVELS, MAX_DECISIONS, MAX_ITERATIONS, MAX_POINTS, NEIGHBOURS = 5, 512, 100, 65536, 10     # the EDS_INI_* constants
FIRST, NEWEST = 0, 1                      # which = ... of level()
JB, JB_NEW = 0, 1                         # which = ... of jb()


class Params(capi.ParamStruct):
    """``eds_ini_params`` — the settings trackFrame reads (reference src/init/CoarseInitializer.cpp:58-61, :79-86)."""
    _fields_ = [("huber_th", C.c_float), ("outlier_th", C.c_float), ("alpha_k", C.c_float), ("alpha_w", C.c_float), ("reg_weight", C.c_float),
                ("coupling_weight", C.c_float), ("fix_affine", C.c_int32), ("max_iterations", C.c_int32 * 5), ("scale_xi_rot", C.c_float),
                ("scale_xi_trans", C.c_float), ("scale_a", C.c_float), ("scale_b", C.c_float)]

    def as_dict(self):
        d = super().as_dict()
        d["max_iterations"] = list(self.max_iterations)
        return d

    def update(self, **over):
        if "max_iterations" in over:
            over = dict(over, max_iterations=(C.c_int32 * 5)(*[int(v) for v in over["max_iterations"]]))
        return super().update(**over)


# eds_ini_point and eds_ini_result as numpy records
POINT = np.dtype([("u", "f4"), ("v", "f4"), ("idepth", "f4"), ("idepth_new", "f4"), ("iR", "f4"), ("lastHessian", "f4"), ("lastHessian_new", "f4"),
                  ("maxstep", "f4"), ("energy", "f4", 2), ("energy_new", "f4", 2), ("my_type", "f4"), ("outlierTH", "f4"), ("isGood", "i4"),
                  ("isGood_new", "i4")])
RESULT = np.dtype([("T", "f8", (3, 4)), ("aff", "f8", 2), ("latest_res", "f4", 3), ("rescale", "f4"), ("snapped", "i4"), ("frame_id", "i4"),
                   ("snapped_at", "i4"), ("ready", "i4"), ("n_decisions", "i4"), ("launches", "i4"), ("waits", "i4"), ("reserved", "i4"),
                   ("iterations", "i4", 5), ("accepts", "i4", 5), ("decisions", "u1", MAX_DECISIONS)])
assert POINT.itemsize == 64 and RESULT.itemsize == 712


@functools.lru_cache(maxsize=None)
def _lib():
    vp, i64, f, i = C.c_void_p, C.c_int64, C.c_float, C.c_int
    return capi.bind(capi.INI_EXPORTS + capi.INISETUP_EXPORTS, {
        "eds_ini_params_default": ([C.POINTER(Params)], None),
        "eds_ini_create": [i] * 5 + [C.POINTER(vp)],
        "eds_ini_destroy": ([vp], None),
        "eds_ini_set_params": [vp, C.POINTER(Params)],
        "eds_ini_get_params": [vp, C.POINTER(Params)],
        "eds_ini_set_calib": [vp, f, f, f, f],
        "eds_ini_set_first": [vp, vp, i64, i, f],
        "eds_ini_set_pose": [vp, vp, vp],
        "eds_ini_set_points": [vp, i, vp, i64, i, vp],
        "eds_ini_set_points_selected": [vp, vp, vp],
        "eds_ini_set_neighbours": [vp, i, vp, vp],
        "eds_ini_make_nn": [i, vp, i, vp, vp, vp],
        "eds_ini_get_schedule_depth": [vp, i, vp],
        "eds_ini_track_frame": [vp, vp, i64, i, f, i, vp],
        "eds_ini_get_kernel_ms": [vp, vp],
        "eds_ini_get_points": [vp, i, vp, vp],
        "eds_ini_get_jb": [vp, i, i, vp],
        "eds_ini_get_level": [vp, i, i, vp],
        # include/eds_hip_inisetup.h
        "eds_ini_setup_abi_version": [],
        "eds_ini_get_sparsity": [vp, vp],
        "eds_ini_set_sparsity": [vp, C.c_int32],
        "eds_ini_make_pixel_status": [vp, i, f, i, f, vp, vp],
        "eds_ini_get_pixel_status": [vp, i, vp],
        "eds_ini_set_points_status": [vp, i, vp],
        "eds_ini_make_neighbours": [vp, i],
        "eds_ini_get_neighbours": [vp, i, vp, vp],
        "eds_ini_get_neighbours_kernel_ms": [vp, vp],
        "eds_ini_setup_levels": [vp, vp, vp, vp],
    })


def default_params(**over) -> Params:
    p = Params()
    _lib().eds_ini_params_default(C.byref(p))
    return p.update(**over)


def make_nn(uv, uv_up=None):
    """``makeNN``'s tables as the reference's nanoflann fills them, ties included (its k-d tree with leaf size 5 and its walk, restated
    in csrc/eds_nntree.hpp and pinned by tests/test_nn_pin.py): the 10 nearest points of the level in nanoflann's order, and with
    `uv_up` (the level above) every point's parent; returns (neighbours n x 10, parent or None)"""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    nb = np.full((len(uv), NEIGHBOURS), -1, np.int32)
    if uv_up is None:
        capi._check(_lib().eds_ini_make_nn(len(uv), _vp(uv), 0, None, _vp(nb), None))
        return nb, None
    up = np.ascontiguousarray(uv_up, dtype=np.float32).reshape(-1, 2)
    parent = np.zeros(len(uv), np.int32)
    capi._check(_lib().eds_ini_make_nn(len(uv), _vp(uv), len(up), _vp(up), _vp(nb), _vp(parent)))
    return nb, parent


_vp = capi.vp


class CoarseInitializer(capi.OwnedHandle):
    """The first frame with one point set per level, and the alignment of every later frame to it, in device memory."""
    _destroy = "eds_ini_destroy"

    def __init__(self, H, W, levels=5, max_points_per_level=16384, device=0, **params):
        self._h = C.c_void_p()
        self.H, self.W, self.levels, self.device = int(H), int(W), int(levels), int(device)
        capi._check(_lib().eds_ini_create(self.device, self.H, self.W, self.levels, int(max_points_per_level), C.byref(self._h)))
        self.n = np.zeros(self.levels, np.int32)
        self.last = None
        if params:
            self.set_params(**params)

    def set_params(self, **over):
        p = self.params().update(**over)
        capi._check(_lib().eds_ini_set_params(self._h, C.byref(p)))

    def params(self) -> Params:
        p = Params()
        capi._check(_lib().eds_ini_get_params(self._h, C.byref(p)))
        return p

    def set_calib(self, fx, fy, cx, cy):
        capi._check(_lib().eds_ini_set_calib(self._h, fx, fy, cx, cy))

    def _plane(self, a, h, w, what):
        """(pointer, row stride in elements, on_device, keep-alive) of an h x w float32 plane in host or device memory"""
        if not capi.is_device_source(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (h, w):
                raise ValueError(f"{what} must be {h} x {w}, not {a.shape}")
            return a.ctypes.data_as(C.c_void_p), 0, 0, a
        ptr, shape, est, dt = capi.device_array_info(a)
        if dt != np.float32 or tuple(shape) != (h, w) or est[1] != 1:
            raise ValueError(f"a device {what} must be float32 {h} x {w} with contiguous rows")
        return C.c_void_p(ptr), int(est[0]), 1, a

    def setFirst(self, image, exposure=1.0):
        """the first frame; thisToNext, snapped, frameID and snappedAt start over.  The points and tables are set_points / set_neighbours."""
        ptr, rs, dev, keep = self._plane(image, self.H, self.W, "image")
        capi._check(_lib().eds_ini_set_first(self._h, ptr, rs, dev, exposure))

    def set_pose(self, T, aff=(0.0, 0.0)):
        """thisToNext (3 x 4 [R | t]) and thisToNext_aff: the guess the next trackFrame starts from"""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(12)
        a = np.ascontiguousarray(aff, dtype=np.float64).reshape(2)
        capi._check(_lib().eds_ini_set_pose(self._h, _vp(T), _vp(a)))

    def set_points(self, lvl, status):
        """one level's points from a status map of the level's size (non-zero: selected, the value is my_type); returns their number"""
        ptr, rs, dev, keep = self._plane(status, self.H >> lvl, self.W >> lvl, "status map")
        n = C.c_int32()
        capi._check(_lib().eds_ini_set_points(self._h, int(lvl), ptr, rs, dev, C.cast(C.byref(n), C.c_void_p)))
        self.n[lvl] = n.value
        return n.value

    def set_points_selected(self, selector):
        """level 0 from the map a ``select.Selector``'s last ``make_maps`` left in device memory"""
        n = C.c_int32()
        capi._check(_lib().eds_ini_set_points_selected(self._h, selector._h, C.cast(C.byref(n), C.c_void_p)))
        self.n[0] = n.value
        return n.value

    def set_neighbours(self, lvl, neighbours, parent=None):
        nb = np.ascontiguousarray(neighbours, dtype=np.int32)
        if nb.shape != (int(self.n[lvl]), NEIGHBOURS):
            raise ValueError(f"neighbours must be {int(self.n[lvl])} x {NEIGHBOURS}, not {nb.shape}")
        par = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
        if par is not None and par.shape != (int(self.n[lvl]),):
            raise ValueError("one parent per point")
        capi._check(_lib().eds_ini_set_neighbours(self._h, int(lvl), _vp(nb), _vp(par)))

    def schedule_depth(self, lvl):
        d = C.c_int32()
        capi._check(_lib().eds_ini_get_schedule_depth(self._h, int(lvl), C.cast(C.byref(d), C.c_void_p)))
        return d.value

    def trackFrame(self, image, exposure=1.0, snapped_threshold=5):
        """trackFrame for one new frame: one kernel launch and one wait; returns a RESULT record (``ready`` is the reference's bool)"""
        ptr, rs, dev, keep = self._plane(image, self.H, self.W, "image")
        out = np.zeros(1, RESULT)
        capi._check(_lib().eds_ini_track_frame(self._h, ptr, rs, dev, exposure, int(snapped_threshold), _vp(out)))
        self.last = out[0]
        return out[0]

    def kernel_ms(self):
        """the device time of the last trackFrame's kernel, in milliseconds"""
        ms = C.c_float()
        capi._check(_lib().eds_ini_get_kernel_ms(self._h, C.cast(C.byref(ms), C.c_void_p)))
        return ms.value

    def rescale(self):
        """|thisToNext.translation()| after the last trackFrame"""
        if self.last is None:
            raise capi.EdsError(capi.ERR_STATE, "rescale() before the first trackFrame")
        return float(self.last["rescale"])

    def points(self, lvl):
        out, n = np.zeros(int(self.n[lvl]), POINT), C.c_int32()
        capi._check(_lib().eds_ini_get_points(self._h, int(lvl), _vp(out) if len(out) else _vp(np.zeros(1, POINT)), C.cast(C.byref(n), C.c_void_p)))
        return out[:n.value]

    def jb(self, lvl, which=JB):
        out = np.zeros((max(int(self.n[lvl]), 1), 10), np.float32)
        capi._check(_lib().eds_ini_get_jb(self._h, int(lvl), int(which), _vp(out)))
        return out[:int(self.n[lvl])]

    def level(self, which, lvl):
        out = np.zeros((self.H >> lvl, self.W >> lvl, 3), np.float32)
        capi._check(_lib().eds_ini_get_level(self._h, int(which), int(lvl), _vp(out)))
        return out

    # ---- include/eds_hip_inisetup.h: the rest of setFirst ----------------------------------------------------------------------------
    @property
    def sparsity(self):
        """the reference's global ``sparsityFactor``: 5 on a new handle, left by every ``make_pixel_status`` as the reference leaves it"""
        v = C.c_int32()
        capi._check(_lib().eds_ini_get_sparsity(self._h, C.cast(C.byref(v), C.c_void_p)))
        return v.value

    @sparsity.setter
    def sparsity(self, value):
        capi._check(_lib().eds_ini_set_sparsity(self._h, int(value)))

    def make_pixel_status(self, lvl, density, recursions_left=5, th_factor=1.0):
        """``makePixelStatus`` of one level of the first frame; the map stays on the device.  Returns (n_good, passes)."""
        n, passes = C.c_int32(), C.c_int32()
        capi._check(_lib().eds_ini_make_pixel_status(self._h, int(lvl), float(density), int(recursions_left), float(th_factor),
                                                     C.cast(C.byref(n), C.c_void_p), C.cast(C.byref(passes), C.c_void_p)))
        return n.value, passes.value

    def pixel_status(self, lvl):
        """the level's map as (H >> lvl) x (W >> lvl) bytes, 0 / 1"""
        out = np.zeros((self.H >> lvl, self.W >> lvl), np.uint8)
        capi._check(_lib().eds_ini_get_pixel_status(self._h, int(lvl), _vp(out)))
        return out

    def set_points_status(self, lvl):
        """the level's points from the map ``make_pixel_status`` left on the device (my_type 1); returns their number"""
        n = C.c_int32()
        capi._check(_lib().eds_ini_set_points_status(self._h, int(lvl), C.cast(C.byref(n), C.c_void_p)))
        self.n[lvl] = n.value
        return n.value

    def make_neighbours(self, lvl=None):
        """``makeNN`` on the device and everything ``set_neighbours`` does with its tables; lvl None: every level, top first"""
        for l in (range(self.levels - 1, -1, -1) if lvl is None else [int(lvl)]):
            capi._check(_lib().eds_ini_make_neighbours(self._h, l))

    def neighbours(self, lvl):
        """the tables ``make_neighbours`` made: (neighbours n x 10, parent n or None at the top level)"""
        n, top = int(self.n[lvl]), int(lvl) == self.levels - 1
        nb, par = np.full((max(n, 1), NEIGHBOURS), -1, np.int32), np.zeros(max(n, 1), np.int32)
        capi._check(_lib().eds_ini_get_neighbours(self._h, int(lvl), _vp(nb), None if top else _vp(par)))
        return nb[:n], None if top else par[:n]

    def neighbours_kernel_ms(self):
        """the device time of the last ``make_neighbours`` level's search kernel, in milliseconds"""
        ms = C.c_float()
        capi._check(_lib().eds_ini_get_neighbours_kernel_ms(self._h, C.cast(C.byref(ms), C.c_void_p)))
        return ms.value

    def setup_levels(self, selector, densities=None):
        """setFirst's points and tables for every level, on the device: `selector` (a ``select.Selector`` of the same size) holds the
        first frame; densities None: the reference's {0.03, 0.05, 0.15, 0.5, 1}.  Returns the points per level."""
        d = None
        if densities is not None:
            d = np.ascontiguousarray(densities, dtype=np.float32).reshape(-1)
            if len(d) < self.levels:
                raise ValueError(f"one density per level: {self.levels}")
        n = np.zeros(MAX_LEVELS, np.int32)
        capi._check(_lib().eds_ini_setup_levels(self._h, selector._h, _vp(d), _vp(n)))
        self.n[:] = n[:self.levels]
        return self.n.copy()
