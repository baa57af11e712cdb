"""ctypes side of tests/host_logic/inisetup_harness.cpp: csrc/eds_inisetup.hpp (gridMaxSelection and makePixelStatus as the host restates
them) and makeNN's tables (edsini::make_nn over csrc/eds_nntree.hpp, and the exhaustive rule it replaced) compiled with g++ into a
temporary directory where the tests run, and the stand-alone program of the same source."""
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
        L.inisetup_make_nn.argtypes = [i, vp, i, vp, i, vp, vp, vp, vp, vp]
        L.inisetup_make_nn_exhaustive.argtypes = [i, vp, i, vp, vp, vp]
        L.inisetup_nn_build.argtypes = [i, vp]
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


def nn_stack():
    """edsnn::STACK: the deepest tree the explicit walk takes"""
    return load_harness().inisetup_nn_stack()


def nn_build(uv):
    """edsnn::build alone — the host work of eds_ini_make_neighbours per level; returns the tree's depth"""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    return load_harness().inisetup_nn_build(len(uv), _vp(uv))


def make_nn(uv, uv_up=None, stack=None):
    """edsini::make_nn — nanoflann's tables as csrc/eds_nntree.hpp restates them.  stack: the deepest tree the explicit walk takes (None:
    edsnn::STACK; 0: every tree with an inner node is walked by recursion).  Returns dict(nb, dist, parent, parent_dist, depth, depth_up);
    parent is -1 and parent_dist 0 without a level above."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    up = np.zeros((0, 2), np.float32) if uv_up is None else np.ascontiguousarray(uv_up, dtype=np.float32).reshape(-1, 2)
    n = len(uv)
    nb, dist = np.full((n, 10), -7, np.int32), np.full((n, 10), -7, np.float32)
    parent, parent_dist, depth = np.full(n, -1, np.int32), np.zeros(n, np.float32), np.zeros(2, np.int32)
    L = load_harness()
    L.inisetup_make_nn(n, _vp(uv), len(up), _vp(up) if len(up) else None, L.inisetup_nn_stack() if stack is None else int(stack), _vp(nb), _vp(dist),
                       _vp(parent) if len(up) else None, _vp(parent_dist), _vp(depth))
    return dict(nb=nb, dist=dist, parent=parent, parent_dist=parent_dist, depth=int(depth[0]), depth_up=int(depth[1]))


def make_nn_exhaustive(uv, uv_up=None):
    """edsini::make_nn_exhaustive — (fp32 squared distance, lower index): (nb, parent or None)"""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    nb = np.full((len(uv), 10), -1, np.int32)
    if uv_up is None:
        load_harness().inisetup_make_nn_exhaustive(len(uv), _vp(uv), 0, None, _vp(nb), None)
        return nb, None
    up = np.ascontiguousarray(uv_up, dtype=np.float32).reshape(-1, 2)
    parent = np.zeros(len(uv), np.int32)
    load_harness().inisetup_make_nn_exhaustive(len(uv), _vp(uv), len(up), _vp(up), _vp(nb), _vp(parent))
    return nb, parent


def run_standalone(extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all) and runs it once"""
    exe, _ = hb.build_program("inisetup", SRC, "INISETUP_STANDALONE", extra_flags)
    return subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/inisetup_harness.py [g++ flags]
    import sys
    print(run_standalone(sys.argv[1:]), end="")
