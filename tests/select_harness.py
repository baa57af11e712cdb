"""ctypes side of tests/host_logic/select_harness.cpp: csrc/eds_pixsel.hpp (namespace edspix, what the device kernels run) compiled with
g++ into a temporary directory where the tests run, and the stand-alone program of the same source with the cases dumped for it.
``HostSelector`` has the interface of ``select.Selector``, so one comparison serves the host restatement and the device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "select_harness.cpp")
PARAM_ORDER = ("min_grad_hist_cut", "min_grad_hist_add", "grad_downweight_per_level", "select_direction_distribution")
_vp = C.c_void_p


def pack_params(prm):
    """eds_sel_params / edspix::Params from the oracle's dict"""
    return struct.pack("<fffi", *(prm[k] for k in PARAM_ORDER))


_lib = None


def load_harness():
    global _lib
    if _lib is None:
        _lib = hb.load_library("select", SRC)
        _lib.sel_new.restype = _vp
        _lib.sel_new.argtypes = [C.c_int, C.c_int]
        _lib.sel_free.argtypes = [_vp]
        _lib.sel_free.restype = None
        _lib.sel_set_params.argtypes = [_vp, C.c_char_p]
        _lib.sel_set_table.argtypes = [_vp, _vp, C.c_size_t]
        _lib.sel_set_potential.argtypes = [_vp, C.c_int]
        _lib.sel_get_potential.argtypes = [_vp]
        _lib.sel_hist_valid.argtypes = [_vp]
        _lib.sel_set_image.argtypes = [_vp, _vp, C.c_int64, _vp]
        _lib.sel_make_maps.argtypes = [_vp, C.c_float, C.c_int, C.c_float, _vp, C.c_int, _vp, _vp]
        _lib.sel_get_map.argtypes = [_vp, _vp]
        _lib.sel_get_level.argtypes = [_vp, C.c_int, _vp]
        _lib.sel_get_thresholds.argtypes = [_vp, C.c_int, _vp]
        _lib.sel_scan_info.argtypes = [_vp, _vp, _vp]
        _lib.sel_selection.argtypes = [_vp, _vp, _vp]
        _lib.sel_fill_reference_pattern.argtypes = [_vp, C.c_size_t]
        assert _lib.sel_params_size() == len(pack_params({k: 0 for k in PARAM_ORDER})) == 16 and _lib.sel_pass_size() == 16
    return _lib


_p = hb.p


def reference_pattern(n):
    out = np.zeros(int(n), np.uint8)
    load_harness().sel_fill_reference_pattern(_p(out), out.size)
    return out


class HostSelector:
    """edspix::Serial behind the interface of slam-eds_amd.select.Selector"""

    def __init__(self, H, W, table=None, **prm):
        import np_select_oracle as so
        self.hl = load_harness()
        self.H, self.W = int(H), int(W)
        self._h = _vp(self.hl.sel_new(self.H, self.W))
        self.passes, self.pass_maps = [], None
        self.hl.sel_set_params(self._h, pack_params(so.params(**prm)))
        if table is not None:
            self.set_random_pattern(table)

    def close(self):
        if getattr(self, "_h", None):
            self.hl.sel_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_random_pattern(self, table):
        t = np.ascontiguousarray(table, np.uint8).reshape(-1)
        self.hl.sel_set_table(self._h, _p(t), t.size)

    @property
    def potential(self):
        return self.hl.sel_get_potential(self._h)

    @potential.setter
    def potential(self, v):
        self.hl.sel_set_potential(self._h, int(v))

    @property
    def hist_valid(self):
        return bool(self.hl.sel_hist_valid(self._h))

    def set_image(self, image, B=None):
        a = np.ascontiguousarray(image, np.float32)
        b = None if B is None else np.ascontiguousarray(B, np.float32)
        self.hl.sel_set_image(self._h, _p(a), self.W, _p(b))

    def make_maps(self, density, recursions_left=1, th_factor=1.0, keep_pass_maps=False):
        cap = int(recursions_left) + 1
        ps = np.zeros((cap, 4), np.int32)
        maps = np.zeros((cap, self.H, self.W), np.uint8) if keep_pass_maps else None
        npass = C.c_int()
        n = self.hl.sel_make_maps(self._h, C.c_float(density), int(recursions_left), C.c_float(th_factor), _p(ps), cap, C.byref(npass), _p(maps))
        self.passes = [tuple(int(v) for v in r) for r in ps[:npass.value]]
        self.pass_maps = None if maps is None else maps[:npass.value]
        return n

    def map(self):
        out = np.zeros((self.H, self.W), np.uint8)
        self.hl.sel_get_map(self._h, _p(out))
        return out

    def selection(self):
        uv, typ = np.zeros((self.H * self.W, 2), np.int32), np.zeros(self.H * self.W, np.float32)
        n = self.hl.sel_selection(self._h, _p(uv), _p(typ))
        return uv[:n].copy(), typ[:n].copy()

    def level(self, lvl):
        out = np.zeros((self.H >> lvl, self.W >> lvl, 4), np.float32)
        self.hl.sel_get_level(self._h, lvl, _p(out))
        return out

    def thresholds(self, which=1):
        out = np.zeros((self.H // 32, self.W // 32), np.float32)
        self.hl.sel_get_thresholds(self._h, int(which), _p(out))
        return out

    def scan_info(self):
        a, c = C.c_int(), C.c_int()
        self.hl.sel_scan_info(self._h, C.byref(a), C.byref(c))
        return a.value, c.value


def dump_cases(path, cases, prm_of):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<5i", c.H, c.W, c.potential, c.recursions, 0 if c.B is None else 1))
            f.write(pack_params(prm_of(c)))
            f.write(struct.pack("<ff", c.density, c.th_factor))
            f.write(np.ascontiguousarray(c.image, np.float32).tobytes())
            f.write(np.ascontiguousarray(c.table, np.uint8).tobytes())
            f.write(np.ascontiguousarray(np.zeros(256) if c.B is None else c.B, np.float32).tobytes())


def run_standalone(cases, prm_of, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own hostile inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("select", SRC, "SEL_STANDALONE", extra_flags)
    dump_cases(data, cases, prm_of)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/select_harness.py [g++ flags]: the sanitizer run of DESIGN §20
    import sys
    sys.path.insert(0, HERE)
    import np_select_oracle as so
    import select_cases as sc
    print(run_standalone(list(sc.cases().values()), lambda c: so.params(**c.prm), sys.argv[1:]), end="")
