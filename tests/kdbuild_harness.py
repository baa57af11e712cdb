"""ctypes side of tests/host_logic/kdbuild_harness.cpp: the product header's serial sort-based build (edskdb::build_sorted), the
nth_element build (edskd::build_tree) and the walk (edskd::nn), compiled with g++ where the tests run."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_logic", "kdbuild_harness.cpp")
LIB = os.path.join(HERE, "host_logic", "libkdbuild.so")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def load_harness():
    deps = [SRC] + [os.path.join(ROOT, "slam-eds_amd", "csrc", f) for f in ("eds_kdbuild.hpp", "eds_kdtree.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", LIB, SRC])
    return C.CDLL(LIB)


def header_sorted(hl, xy):
    """(perm or None, ambiguous) of edskdb::build_sorted"""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    perm = np.zeros(max(len(xy), 1), dtype=np.int32)
    ok = hl.kdb_build_sorted(xy.ctypes.data_as(_dp), len(xy), perm.ctypes.data_as(_ip))
    return (perm[:len(xy)].astype(np.int64), False) if ok else (None, True)


def host_tree(hl, xy):
    """edskd::build_tree's index array"""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    perm = np.zeros(max(len(xy), 1), dtype=np.int32)
    hl.kdb_build_tree(xy.ctypes.data_as(_dp), len(xy), perm.ctypes.data_as(_ip))
    return perm[:len(xy)].astype(np.int64)


def walk(hl, txy, q):
    txy, q = np.ascontiguousarray(txy, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    pos, dist = np.zeros(len(q), dtype=np.int32), np.zeros(len(q))
    hl.kdb_nn(txy.ctypes.data_as(_dp), len(txy), q.ctypes.data_as(_dp), len(q), pos.ctypes.data_as(_ip), dist.ctypes.data_as(_dp))
    return pos.astype(np.int64), dist
