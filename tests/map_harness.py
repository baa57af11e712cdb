"""ctypes side of tests/host_logic/map_harness.cpp: csrc/eds_map.hpp (namespace edsmap, what the device kernels run) compiled with g++
into a temporary directory where the tests run; the functions here have the results of ``np_map_oracle``'s, so one comparison serves both.
``standalone`` builds the program of the same source and dumps cases for it."""
import ctypes as C
import os
import struct

import numpy as np

import harness_build as hb

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "map_harness.cpp")
_p = hb.p
_lib = None


def load_harness():
    global _lib
    if _lib is None:
        L = hb.load_library("map", SRC)
        vp, i, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
        a, b = C.c_int(), C.c_int()
        assert L.map_sizes(C.byref(a), C.byref(b)) == 16 and a.value == 8
        L.map_window_cloud.restype = i64
        L.map_window_cloud.argtypes = [i, vp, vp, vp, vp, i, u32, vp, i, vp, vp]
        L.map_window_depth_maps.argtypes = [i, vp, vp, vp, vp, i, u32, vp, i, vp, vp, i, i, i64, vp, vp, vp, vp]
        L.map_immature_cloud.restype = i64
        L.map_immature_cloud.argtypes = [i, u32, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp]
        L.map_slot_cloud.restype = None
        L.map_slot_cloud.argtypes = [i, vp, vp, vp, vp, vp]
        L.chunk = b.value
        _lib = L
    return _lib


def chunk():
    """the compacting kernels' workgroup size: points per sweep"""
    return load_harness().chunk


def _win(host, uv, ids, calib, T_w_c):
    return (np.ascontiguousarray(host, np.int32), np.ascontiguousarray(uv, np.float32).reshape(-1, 2), np.ascontiguousarray(ids, np.float32),
            np.ascontiguousarray(calib, np.float32), np.ascontiguousarray(T_w_c, np.float64).reshape(-1, 12))


def window_cloud(host, uv, ids, calib, T_w_c, mask, single_point):
    host, uv, ids, calib, T = _win(host, uv, ids, calib, T_w_c)
    pts, per = np.zeros((len(host) * (1 if single_point else 8), 3)), np.zeros(8, np.int32)
    n = load_harness().map_window_cloud(len(host), _p(host), _p(uv), _p(ids), _p(calib), len(T), mask, _p(T), 1 if single_point else 0, _p(pts), _p(per))
    assert n >= 0
    return pts[:n], per


def window_depth_maps(host, uv, ids, calib, T_w_c, mask, T_dst_w, K_dst, dst_H, dst_W):
    host, uv, ids, calib, T = _win(host, uv, ids, calib, T_w_c)
    Td, K = np.ascontiguousarray(T_dst_w, np.float64).reshape(-1, 12), np.ascontiguousarray(K_dst, np.float64).reshape(-1, 4)
    count, stride = len(Td), max(len(host), 1)
    xy, idp, src, n = np.zeros((count, stride, 2)), np.zeros((count, stride)), np.zeros((count, stride), np.int32), np.zeros(count, np.int32)
    assert load_harness().map_window_depth_maps(len(host), _p(host), _p(uv), _p(ids), _p(calib), len(T), mask, _p(T), count, _p(Td), _p(K), dst_H, dst_W,
                                                stride, _p(xy), _p(idp), _p(src), _p(n)) == 0
    return [dict(xy=xy[b, :n[b]], idp=idp[b, :n[b]], src=src[b, :n[b]]) for b in range(count)]


def immature_cloud(n_per_host, uv, idepth_min, idepth_max, status, alive, T_w_c, calib, mask, single_point):
    first = np.concatenate([[0], np.cumsum(n_per_host)]).astype(np.int32)
    total = int(first[-1])
    uv, lo, hi = (np.ascontiguousarray(a, np.float32) for a in (uv, idepth_min, idepth_max))
    st, al = np.ascontiguousarray(status, np.int32), np.ascontiguousarray(alive, np.int32)
    T, cal = np.ascontiguousarray(T_w_c, np.float64).reshape(-1, 12), np.ascontiguousarray(calib, np.float32)
    cap = max(total, 1) * (1 if single_point else 8)
    pts, col, so = np.zeros((cap, 3)), np.zeros((cap, 4)), np.zeros(cap, np.uint8)
    n = load_harness().map_immature_cloud(len(T), mask, _p(first), _p(uv), _p(lo), _p(hi), _p(st), _p(al), _p(T), _p(cal), 1 if single_point else 0,
                                          _p(pts), _p(col), _p(so))
    return dict(points=pts[:n], colors=col[:n], status=so[:n])


def slot_cloud(xn, yn, idp, T_w_kf):
    xn, yn, idp = np.ascontiguousarray(xn, np.float32), np.ascontiguousarray(yn, np.float32), np.ascontiguousarray(idp, np.float64)
    T, out = np.ascontiguousarray(T_w_kf, np.float64).reshape(12), np.zeros((len(xn), 3))
    load_harness().map_slot_cloud(len(xn), _p(xn), _p(yn), _p(idp), _p(T), _p(out))
    return out


def standalone(cases, extra_flags=()):
    """the stand-alone program of the harness source, and the case file written for it: (program, file)"""
    exe, data = hb.build_program("map", SRC, "MAP_STANDALONE", extra_flags)
    with open(data, "wb") as f:
        for c in cases:
            host, uv, ids, calib, T = _win(c["host"], c["uv"], c["ids"], c["calib"], c["T_w_c"])
            Td, K = np.ascontiguousarray(c["T_dst_w"], np.float64), np.ascontiguousarray(c["K_dst"], np.float64)
            f.write(struct.pack("<6i", len(host), len(T), c["mask"] & 0x7FFFFFFF, len(Td), c["dst_H"], c["dst_W"]))
            for a in (host, uv, ids, calib, T, Td, K):
                f.write(a.tobytes())
    return exe, data
