"""ctypes side of tests/host_logic/inisetup_harness.cpp: csrc/eds_inisetup.hpp (gridMaxSelection and makePixelStatus as the host restates
them) compiled with g++ into a temporary directory where the tests run, and the stand-alone program of the same source."""
import ctypes as C
import subprocess

import numpy as np

import harness_build as hb
import init_harness as ih

SRC = ih.SRC.replace("init_harness.cpp", "inisetup_harness.cpp")
_lib = None
_vp = hb.p


def load_harness():
    global _lib
    if _lib is None:
        L = hb.load_library("inisetup", SRC)
        vp, f, i = C.c_void_p, C.c_float, C.c_int
        L.inisetup_cells.argtypes = [i, i]
        L.inisetup_grid_max_selection.argtypes = [vp, i, i, i, f, vp]
        L.inisetup_make_pixel_status.argtypes = [vp, i, i, f, i, f, vp, vp, vp]
        _lib = L
    return _lib


def cells(w, pot):
    return load_harness().inisetup_cells(int(w), int(pot))


def grid_max_selection(grads, pot, th_fac):
    """grads h x w x {colour, dx, dy}; returns (map, numGood)"""
    g = np.ascontiguousarray(grads, dtype=np.float32)
    h, w = g.shape[:2]
    status = np.full((h, w), 255, np.uint8)
    n = load_harness().inisetup_grid_max_selection(_vp(g), w, h, int(pot), float(th_fac), _vp(status))
    return status, n


def make_pixel_status(grads, desired, recs_left, th_fac, sparsity):
    """returns (map, numGoodPoints, passes, the sparsity left behind)"""
    g = np.ascontiguousarray(grads, dtype=np.float32)
    h, w = g.shape[:2]
    status = np.full((h, w), 255, np.uint8)
    sp, passes = np.array([sparsity], np.int32), np.zeros(1, np.int32)
    n = load_harness().inisetup_make_pixel_status(_vp(g), w, h, float(desired), int(recs_left), float(th_fac), _vp(sp), _vp(passes), _vp(status))
    return status, n, int(passes[0]), int(sp[0])


def run_standalone(extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all) and runs it once"""
    exe, _ = hb.build_program("inisetup", SRC, "INISETUP_STANDALONE", extra_flags)
    return subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/inisetup_harness.py [g++ flags]
    import sys
    print(run_standalone(sys.argv[1:]), end="")
