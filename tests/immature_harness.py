"""ctypes side of tests/host_logic/immature_harness.cpp: csrc/eds_immature.hpp (namespace edsimm, what the device kernels run) compiled
with g++ into a temporary directory where the tests run, and the stand-alone program of the same source with the cases dumped for it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_logic", "immature_harness.cpp")
_fp = C.POINTER(C.c_float)

# edsimm::Point, 32 words
POINT = np.dtype([("color", "f4", 8), ("weights", "f4", 8), ("gradH", "f4", 4), ("energyTH", "f4"), ("u", "f4"), ("v", "f4"), ("quality", "f4"),
                  ("idepth_min", "f4"), ("idepth_max", "f4"), ("last_uv", "f4", 2), ("last_interval", "f4"), ("type", "f4"), ("status", "i4"),
                  ("alive", "i4")])
PARAM_ORDER = ("max_pix_search", "trace_stepsize", "trace_gn_iterations", "trace_gn_threshold", "trace_extra_slack_on_th", "trace_slack_interval",
               "trace_min_improvement_factor", "min_trace_test_radius", "huber_th", "outlier_th", "outlier_th_sum_component",
               "overall_energy_th_weight")
_INT = ("trace_gn_iterations", "min_trace_test_radius")


def pack_params(prm):
    """eds_imm_params / edsimm::Params from the oracle's dict"""
    return b"".join(struct.pack("<i" if k in _INT else "<f", prm[k]) for k in PARAM_ORDER)


_lib = None


def load_harness():
    global _lib
    if _lib is None:
        _lib = hb.load_library("immature", SRC)
        assert _lib.imm_point_size() == POINT.itemsize == 128
    return _lib


def make_image(hl, color):
    color = np.ascontiguousarray(color, dtype=np.float32)
    H, W = color.shape
    out = np.zeros((H, W, 3), np.float32)
    hl.imm_make_image(color.ctypes.data_as(_fp), H, W, out.ctypes.data_as(_fp))
    return out


def construct(hl, color, uv, typ, idepth, distance, prm):
    color = np.ascontiguousarray(color, dtype=np.float32)
    H, W = color.shape
    uv = np.ascontiguousarray(uv, dtype=np.int32)
    typ = np.ascontiguousarray(typ, dtype=np.float32)
    pts = np.zeros(len(uv), POINT)
    idp = None if idepth is None else np.ascontiguousarray(idepth, dtype=np.float32)
    dist = None if distance is None else np.ascontiguousarray(distance, dtype=np.float64)
    hl.imm_construct(color.ctypes.data_as(_fp), H, W, pack_params(prm), len(uv), uv.ctypes.data_as(C.c_void_p), typ.ctypes.data_as(_fp),
                     None if idp is None else idp.ctypes.data_as(C.c_void_p), None if dist is None else dist.ctypes.data_as(C.c_void_p),
                     pts.ctypes.data_as(C.c_void_p))
    return pts


def trace(hl, pts, color, prm, KRKi, Kt, aff):
    """traceOn for every point of pts (modified in place) on the frame whose colour plane is `color`"""
    color = np.ascontiguousarray(color, dtype=np.float32)
    H, W = color.shape
    k, t, a = (np.ascontiguousarray(x, dtype=np.float32) for x in (KRKi, Kt, aff))
    hl.imm_trace(pts.ctypes.data_as(C.c_void_p), len(pts), color.ctypes.data_as(_fp), H, W, pack_params(prm), k.ctypes.data_as(_fp),
                 t.ctypes.data_as(_fp), a.ctypes.data_as(_fp))


def gradient(hl, color):
    """the frame's gradient plane (H x W x 2), for trace_g"""
    color = np.ascontiguousarray(color, dtype=np.float32)
    g = np.zeros(color.shape + (2,), np.float32)
    hl.imm_gradient(color.ctypes.data_as(_fp), color.shape[0], color.shape[1], g.ctypes.data_as(_fp))
    return g


def trace_g(hl, pts, color, grad, prm_bytes, KRKi, Kt, aff):
    """trace() on a contiguous slice of points with the gradient plane given: callable from several threads (ctypes drops the GIL)"""
    assert pts.flags["C_CONTIGUOUS"] and color.dtype == np.float32 and grad.dtype == np.float32
    k, t, a = (np.ascontiguousarray(x, dtype=np.float32) for x in (KRKi, Kt, aff))
    hl.imm_trace_g(pts.ctypes.data_as(C.c_void_p), len(pts), color.ctypes.data_as(_fp), grad.ctypes.data_as(_fp), color.shape[0], color.shape[1],
                   prm_bytes, k.ctypes.data_as(_fp), t.ctypes.data_as(_fp), a.ctypes.data_as(_fp))


def line_steps(hl, pts, H, W, prm, KRKi, Kt):
    """numSteps of every point's discrete search (0: it leaves before the search)"""
    k, t = (np.ascontiguousarray(x, dtype=np.float32) for x in (KRKi, Kt))
    out = np.zeros(len(pts), np.int32)
    hl.imm_line_steps(pts.ctypes.data_as(C.c_void_p), len(pts), H, W, pack_params(prm), k.ctypes.data_as(_fp), t.ctypes.data_as(_fp),
                      out.ctypes.data_as(C.c_void_p))
    return out


def dump_cases(path, cases, params_of):
    """the binary the stand-alone program reads: every case's frames, points and per-trace inputs"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<4i", c.H, c.W, len(c.hosts), len(c.targets)))
            f.write(pack_params(params_of(c)))
            for h in c.hosts:
                f.write(np.ascontiguousarray(h["image"], dtype=np.float32).tobytes())
                f.write(struct.pack("<2i", len(h["uv"]), 0 if h["idepth"] is None else 1))
                f.write(np.ascontiguousarray(h["uv"], dtype=np.int32).tobytes())
                f.write(np.ascontiguousarray(h["type"], dtype=np.float32).tobytes())
                if h["idepth"] is not None:
                    f.write(np.ascontiguousarray(h["idepth"], dtype=np.float32).tobytes())
                    f.write(np.ascontiguousarray(h["distance"], dtype=np.float64).tobytes())
            for t in c.targets:
                f.write(np.ascontiguousarray(t, dtype=np.float32).tobytes())
            for step in c.steps:
                for KRKi, Kt, aff, _ in step:
                    f.write(np.concatenate([np.ravel(KRKi), np.ravel(Kt), np.ravel(aff)]).astype(np.float32).tobytes())


def run_standalone(cases, params_of, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own degenerate inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("immature", SRC, "IMM_STANDALONE", extra_flags)
    dump_cases(data, cases, params_of)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/immature_harness.py [g++ flags]: the sanitizer run of DESIGN §15
    import sys
    sys.path.insert(0, HERE)
    import immature_cases as ic
    import np_immature_oracle as no
    print(run_standalone(list(ic.cases().values()), lambda c: no.params(**c.prm), sys.argv[1:]), end="")
