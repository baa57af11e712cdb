"""ctypes side of tests/host_logic/coarse_harness.cpp: csrc/eds_coarse.hpp (namespace edsct, what the device kernels run) compiled with
g++ into a temporary directory where the tests run — ``HostTracker`` has the methods of ``slam-eds_amd.coarse.CoarseTracker`` — and the
stand-alone program of the same source with the cases dumped for it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_logic", "coarse_harness.cpp")
PARAM_ORDER = ("huber_th", "coarse_cutoff_th", "affine_opt_mode_a", "affine_opt_mode_b")
REF_IMAGE, NEW_IMAGE, IDEPTH, WEIGHT_SUMS, PC = range(5)

# edsct::TrackOut / eds_ct_result and edsct::Term / eds_ct_row
RESULT = np.dtype([("T", "f8", (3, 4)), ("aff", "f8", 2), ("last_residuals", "f8", 5), ("last_flow_indicators", "f8", 3), ("ok", "i4"),
                   ("n_decisions", "i4"), ("iterations", "i4", 5), ("accepts", "i4", 5), ("level_cutoff_repeat", "f4"), ("reserved", "i4"),
                   ("decisions", "u1", 512)])
ROW = np.dtype([("in_e", "i4"), ("warped", "i4"), ("flow", "i4"), ("energy", "f4"), ("idepth", "f4"), ("u", "f4"), ("v", "f4"), ("dx", "f4"),
                ("dy", "f4"), ("residual", "f4"), ("weight", "f4"), ("ref_color", "f4"), ("shift_t_pos", "f4"), ("shift_t_neg", "f4"),
                ("shift_rt_pos", "f4"), ("shift_rt_neg", "f4")])


def pack_params(prm):
    return b"".join(struct.pack("<f", prm[k]) for k in PARAM_ORDER)


_lib = None


def load_harness():
    global _lib
    if _lib is None:
        L = hb.load_library("coarse", SRC)
        a, b = C.c_int(), C.c_int()
        assert L.ct_sizes(C.byref(a), C.byref(b)) == 512 and a.value == ROW.itemsize == 64 and b.value == RESULT.itemsize
        vp, f, d = C.c_void_p, C.c_float, C.c_double
        L.ct_create.restype = vp
        L.ct_create.argtypes = [C.c_int] * 3
        L.ct_destroy.argtypes = [vp]
        L.ct_set_params.argtypes = [vp, vp]
        L.ct_set_calib.argtypes = [vp, f, f, f, f]
        L.ct_get_k.argtypes = [vp, C.c_int, vp]
        L.ct_set_ref.argtypes = [vp, vp, f, d, d, C.c_int, vp, vp, vp]
        L.ct_set_new.argtypes = [vp, vp, f]
        L.ct_track.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
        L.ct_calc_res.argtypes = [vp, C.c_int, vp, vp, f, vp, vp, vp, vp]
        L.ct_get_level.argtypes = [vp, C.c_int, C.c_int, vp]
        L.ct_sincos_n.argtypes = [vp, C.c_int, vp, vp]
        L.ct_exp_n.argtypes = [vp, C.c_int, vp]
        _lib = L
    return _lib


_vp = hb.p


def sincos(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    s, c = np.zeros_like(x), np.zeros_like(x)
    load_harness().ct_sincos_n(_vp(x), x.size, _vp(s), _vp(c))
    return s, c


def exp(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    e = np.zeros_like(x)
    load_harness().ct_exp_n(_vp(x), x.size, _vp(e))
    return e


class HostTracker:
    """edsct:: under g++ behind the interface of slam-eds_amd.coarse.CoarseTracker"""

    def __init__(self, H, W, levels=5, **params):
        self.L = load_harness()
        self.H, self.W, self.levels = H, W, levels
        self._h = self.L.ct_create(H, W, levels)
        assert self._h, "shape refused"
        self.prm = dict(huber_th=9.0, coarse_cutoff_th=20.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8)
        self.pc_n = np.zeros(levels, np.int32)
        if params:
            self.set_params(**params)

    def close(self):
        if self._h:
            self.L.ct_destroy(self._h)
            self._h = None

    def set_params(self, **over):
        self.prm.update(over)
        self.L.ct_set_params(self._h, pack_params(self.prm))

    def set_calib(self, fx, fy, cx, cy):
        self.L.ct_set_calib(self._h, fx, fy, cx, cy)

    def K(self, lvl):
        out = np.zeros(4, np.float32)
        self.L.ct_get_k(self._h, lvl, _vp(out))
        return out

    def set_ref(self, image, center_projected, hdif, exposure=1.0, aff=(0.0, 0.0)):
        img = np.ascontiguousarray(image, dtype=np.float32)
        cp = np.ascontiguousarray(center_projected, dtype=np.float32).reshape(-1, 3)
        hd = np.ascontiguousarray(hdif, dtype=np.float32).reshape(-1)
        pc_n = np.zeros(self.levels, np.int32)
        dropped = self.L.ct_set_ref(self._h, _vp(img), exposure, float(aff[0]), float(aff[1]), len(cp), _vp(cp), _vp(hd), _vp(pc_n))
        self.pc_n = pc_n
        return pc_n, dropped

    def set_new(self, image, exposure=1.0):
        self.L.ct_set_new(self._h, _vp(np.ascontiguousarray(image, dtype=np.float32)), exposure)

    def track(self, T_init, aff_init=None, coarsest_lvl=None, min_res_for_abort=None):
        T = np.ascontiguousarray(T_init, dtype=np.float64).reshape(-1, 12)
        a = np.zeros((len(T), 2)) if aff_init is None else np.ascontiguousarray(aff_init, dtype=np.float64).reshape(-1, 2)
        lvl = self.levels - 1 if coarsest_lvl is None else int(coarsest_lvl)
        mr = np.full(5, np.nan) if min_res_for_abort is None else np.ascontiguousarray(min_res_for_abort, dtype=np.float64)
        out = np.zeros(len(T), RESULT)
        self.L.ct_track(self._h, len(T), _vp(T), _vp(a), lvl, _vp(mr), _vp(out))
        return out

    def calc_res(self, lvl, T, aff=(0.0, 0.0), cutoff=None, rows=True):
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(12)
        a = np.ascontiguousarray(aff, dtype=np.float64).reshape(2)
        cutoff = self.prm["coarse_cutoff_th"] if cutoff is None else cutoff
        rs, H, b = np.zeros(6), np.zeros((8, 8)), np.zeros(8)
        r = np.zeros(int(self.pc_n[lvl]), ROW) if rows else None
        self.L.ct_calc_res(self._h, lvl, _vp(T), _vp(a), cutoff, _vp(rs), _vp(H), _vp(b), _vp(r))
        return dict(rs=rs, H=H, b=b, rows=r)

    def level(self, which, lvl):
        w, h = self.W >> lvl, self.H >> lvl
        shape = {REF_IMAGE: (h, w, 3), NEW_IMAGE: (h, w, 3), IDEPTH: (h, w), WEIGHT_SUMS: (h, w), PC: (h * w, 4)}[which]
        out = np.zeros(shape, np.float32)
        n = self.L.ct_get_level(self._h, which, lvl, _vp(out))
        return out[:n] if which == PC else out


def open_case(c, cls=HostTracker, **kw):
    """a tracker of class `cls` holding case c's calibration, parameters and two frames"""
    t = cls(c.H, c.W, c.levels, **kw)
    t.set_params(**c.prm)
    t.set_calib(*c.K)
    t.set_ref(c.ref, c.cp, c.hdif, c.exposure_ref, c.aff_ref)
    t.set_new(c.new, c.exposure_new)
    return t


def dump_cases(path, cases):
    """the binary the stand-alone program reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            prm = dict(huber_th=9.0, coarse_cutoff_th=20.0, affine_opt_mode_a=1e12, affine_opt_mode_b=1e8)
            prm.update(c.prm)
            f.write(struct.pack("<3i", c.H, c.W, c.levels) + pack_params(prm) + struct.pack("<4f", *c.K))
            f.write(np.ascontiguousarray(c.ref, dtype=np.float32).tobytes())
            f.write(struct.pack("<fddi", c.exposure_ref, c.aff_ref[0], c.aff_ref[1], len(c.hdif)))
            f.write(np.ascontiguousarray(c.cp, dtype=np.float32).tobytes() + np.ascontiguousarray(c.hdif, dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(c.new, dtype=np.float32).tobytes())
            T = np.ascontiguousarray(c.T_init, dtype=np.float64).reshape(-1, 12)
            f.write(struct.pack("<fii", c.exposure_new, len(T), c.coarsest))
            f.write(T.tobytes() + np.ascontiguousarray(c.aff_init, dtype=np.float64).tobytes() + np.ascontiguousarray(c.min_res, dtype=np.float64).tobytes())


def run_standalone(cases, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own hostile inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("coarse", SRC, "CT_STANDALONE", extra_flags)
    dump_cases(data, cases)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/coarse_harness.py [g++ flags]: the sanitizer run of DESIGN §16
    import sys
    sys.path.insert(0, HERE)
    import coarse_cases as cc
    print(run_standalone(list(cc.cases().values()), sys.argv[1:]), end="")
