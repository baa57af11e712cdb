"""ctypes side of tests/host_logic/immdepth_harness.cpp: csrc/eds_immdepth.hpp (namespace edsimd, what the device kernels run) compiled
with g++ into a temporary directory where the tests run, and the stand-alone program of the same source with the cases dumped for it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb
from immature_harness import POINT, pack_params

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "immdepth_harness.cpp")
_vp = hb.p
_lib = None


def load_harness():
    global _lib
    if _lib is None:
        _lib = hb.load_library("immdepth", SRC)
        assert _lib.imd_point_size() == POINT.itemsize == 128
    return _lib


def _xy(xy):
    return np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)


def build_tree(hl, xy):
    """edskd::build_tree's index array"""
    xy = _xy(xy)
    perm = np.zeros(max(len(xy), 1), np.int32)
    hl.imd_build_tree(_vp(xy), len(xy), _vp(perm))
    return perm[:len(xy)]


def device_builds(hl, xy):
    """True where the device builds the tree of this map: within the capacity, finite and unambiguous"""
    xy = _xy(xy)
    if len(xy) > hl.imd_capacity():
        return False
    perm = np.zeros(max(len(xy), 1), np.int32)
    return bool(hl.imd_build_sorted(_vp(xy), len(xy), _vp(perm)))


def tree_of(hl, xy, idp):
    """(perm, txy, tidp): the map in tree order"""
    xy, idp = _xy(xy), np.ascontiguousarray(idp, dtype=np.float64)
    perm = build_tree(hl, xy)
    return perm, np.ascontiguousarray(xy[perm]), np.ascontiguousarray(idp[perm])


def _scale(scale):
    return (1.0, 1.0) if scale is None else (float(scale[0]), float(scale[1]))


def nearest(hl, tree, uv, scale=None):
    """steps 1 to 4: dict(pos, index, idepth, distance)"""
    perm, txy, tidp = tree
    uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
    n = len(uv)
    o = dict(pos=np.zeros(n, np.int32), index=np.zeros(n, np.int32), idepth=np.zeros(n, np.float32), distance=np.zeros(n, np.float64))
    sx, sy = _scale(scale)
    hl.imd_nearest(_vp(txy), _vp(tidp), _vp(perm), len(perm), n, _vp(uv), C.c_double(sx), C.c_double(sy), _vp(o["pos"]),
                   _vp(o["index"]), _vp(o["idepth"]), _vp(o["distance"]))
    return o


def _loop(fn, color, prm, tree, uv, typ, scale):
    perm, txy, tidp = tree
    color = np.ascontiguousarray(color, dtype=np.float32)
    H, W = color.shape
    uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
    typ = np.ascontiguousarray(typ, dtype=np.float32)
    n = len(uv)
    pts = np.zeros(n, POINT)
    o = dict(index=np.zeros(n, np.int32), idepth=np.zeros(n, np.float32), distance=np.zeros(n, np.float64))
    sx, sy = _scale(scale)
    fn(_vp(color), H, W, pack_params(prm), _vp(txy), _vp(tidp), _vp(perm), len(perm), n, _vp(uv), _vp(typ), C.c_double(sx), C.c_double(sy), _vp(pts),
       _vp(o["index"]), _vp(o["idepth"]), _vp(o["distance"]))
    return pts, o


def seed(hl, color, prm, tree, uv, typ, scale=None):
    """edsimd::seed for every pixel: (points, dict(index, idepth, distance))"""
    return _loop(hl.imd_seed, color, prm, tree, uv, typ, scale)


def composed(hl, color, prm, tree, uv, typ, scale=None):
    """the same loop from edskd::nn and edsimm::construct alone"""
    return _loop(hl.imd_composed, color, prm, tree, uv, typ, scale)


def dump_cases(path, cases, params_of):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            H, W = c.image.shape
            sx, sy = _scale(c.scale)
            f.write(struct.pack("<4i", H, W, len(c.xy), len(c.uv)))
            f.write(struct.pack("<2d", sx, sy))
            f.write(pack_params(params_of(c)))
            f.write(np.ascontiguousarray(c.image, dtype=np.float32).tobytes())
            f.write(_xy(c.xy).tobytes())
            f.write(np.ascontiguousarray(c.idp, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(c.uv, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(c.type, dtype=np.float32).tobytes())


def run_standalone(cases, params_of, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own degenerate inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("immdepth", SRC, "IMD_STANDALONE", extra_flags)
    dump_cases(data, cases, params_of)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/immdepth_harness.py [g++ flags]: the sanitizer run of the stand-alone program
    import sys
    sys.path.insert(0, HERE)
    import immdepth_cases as dc
    import np_immature_oracle as no
    print(run_standalone(list(dc.cases().values()), lambda c: no.params(), sys.argv[1:]), end="")
