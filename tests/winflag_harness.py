"""ctypes side of tests/host_logic/winflag_harness.cpp: csrc/eds_winflag.hpp (namespace edswfl, what the device kernels run) compiled
with g++ — the functions of tests/np_winflag_oracle.py with the same arguments and results —, and the stand-alone program of the same
source."""
import ctypes as C
import os
import subprocess

import numpy as np

import harness_build as hb
import np_winflag_oracle as oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "winflag_harness.cpp")
_lib = None
_vp = hb.p


def load_harness():
    global _lib
    if _lib is None:
        L = hb.load_library("winflag", SRC)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.wfl_defaults.argtypes = [i, i] + [vp] * 5
        L.wfl_activated.argtypes = [i, i] + [vp] * 5
        L.wfl_forget.argtypes = [i] + [vp] * 4
        L.wfl_frames_down.argtypes = [i, i, vp]
        L.wfl_insert_frame.argtypes = [i, i, i, i] + [vp] * 12
        L.wfl_rel_baseline.argtypes = [vp, f, f, f]
        L.wfl_rel_baseline.restype = f
        L.wfl_apply_fixed.argtypes = [i, i] + [vp] * 13 + [i, vp]
        L.wfl_flag_points.argtypes = [i] + [vp] * 9 + [C.c_uint32, i, vp, vp, vp]
        L.wfl_flag_points.restype = None
        for name in ("wfl_defaults", "wfl_activated", "wfl_forget", "wfl_frames_down", "wfl_apply_fixed"):
            getattr(L, name).restype = None
        _lib = L
    return _lib


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _own(hist):
    """a writable contiguous copy of every column"""
    return dict(num_good=_i32(hist["num_good"]).copy(), max_rel_baseline=_f32(hist["max_rel_baseline"]).copy(), last_target=_i32(hist["last_target"]).copy(),
                last_state=_i32(hist["last_state"]).copy(), is_new=_i32(hist["is_new"]).copy())


def _first(point, n):
    """res_first from the residuals' points (the oracle's runs() without its loop: tools/winflag_measure.py times callers of this)"""
    return _i32(np.concatenate([[0], np.cumsum(np.bincount(np.asarray(point, np.int64), minlength=n))]))


def defaults(n, m):
    h = dict(num_good=np.empty(n, np.int32), max_rel_baseline=np.empty(n, np.float32), last_target=np.empty((n, 2), np.int32),
             last_state=np.empty((n, 2), np.int32), is_new=np.empty(m, np.int32))
    load_harness().wfl_defaults(n, m, *(_vp(h[k]) for k in oracle.COLUMNS))
    return h


def activated(hist_rows, target_mask, F):
    K = len(target_mask)
    h = defaults(K, 0)
    mask = np.ascontiguousarray(target_mask, dtype=np.uint64)
    load_harness().wfl_activated(K, int(F), _vp(mask), *(_vp(h[k]) for k in oracle.COLUMNS[:4]))
    return h


def remove_residuals(hist, point, target, keep_r):
    h = _own(hist)
    keep = _i32(np.asarray(keep_r) != 0)
    load_harness().wfl_forget(len(point), _vp(keep), _vp(_i32(point)), _vp(_i32(target)), _vp(h["last_target"]))
    h["is_new"] = h["is_new"][np.flatnonzero(keep)]             # the gather of csrc/eds_winedit.hpp: a copy
    return h


def remove_points(hist, point, keep_p):
    return oracle.remove_points(hist, point, keep_p)            # copies only: the gather of csrc/eds_winedit.hpp


def marginalize_frame(hist, point, target, frame):
    h = remove_residuals(hist, point, target, np.asarray(target) != frame)
    load_harness().wfl_frames_down(len(h["num_good"]), int(frame), _vp(h["last_target"]))
    return h


def insert_frame_residuals(hist, host, point, target, frame, capacity=None):
    n, m = len(host), len(point)
    h = _own(hist)
    need, map_r = np.zeros(n, np.int32), np.zeros(m + n, np.int32)
    pn, tn, nn = np.zeros(m + n, np.int32), np.zeros(m + n, np.int32), np.zeros(m + n, np.int32)
    K = load_harness().wfl_insert_frame(n, m, int(frame), m + n if capacity is None else int(capacity), _vp(_i32(host)), _vp(_first(point, n)), _vp(_i32(point)),
                                        _vp(_i32(target)), _vp(h["is_new"]), _vp(h["last_target"]), _vp(h["last_state"]), _vp(need), _vp(map_r), _vp(pn),
                                        _vp(tn), _vp(nn))
    if K < 0:
        return None
    h["is_new"] = nn[:m + K].copy()
    return pn[:m + K].copy(), tn[:m + K].copy(), map_r[:m + K].copy(), h


def rel_baseline(pc, u, v, idepth):
    return np.float32(load_harness().wfl_rel_baseline(_vp(_f32(pc)), float(u), float(v), float(idepth)))


def apply_fixed(hist, host, uv, idepth, point, target, state, active, precalc, F, clear_is_new):
    n = len(host)
    h = _own(hist)
    counts = np.zeros(3, np.int32)
    load_harness().wfl_apply_fixed(n, int(F), _vp(_f32(precalc)), _vp(_i32(host)), _vp(_f32(uv)), _vp(_f32(idepth)), _vp(_first(point, n)), _vp(_i32(target)),
                                   _vp(_i32(state)), _vp(_i32(active)), *(_vp(h[k]) for k in oracle.COLUMNS), int(bool(clear_is_new)), _vp(counts))
    return h, counts


def flag_points(hist, host, idepth, point, target, state, idepth_hessian, frames_to_marg, only_empty=False, prm=None):
    """(fates, counts[27], candidates)"""
    n = len(host)
    p = dict(oracle.PARAMS, **(prm or {}))
    prm4 = np.zeros(4, np.int32)
    prm4[0], prm4[1] = p["min_good_active_res_for_marg"], p["min_good_res_for_marg"]
    prm4[2:3] = np.array([p["min_idepth_h_marg"]], np.float32).view(np.int32)
    fate, cand, counts = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(27, np.int32)
    load_harness().wfl_flag_points(n, _vp(prm4), _vp(_i32(hist["num_good"])), _vp(_i32(hist["last_state"])), _vp(_i32(host)), _vp(_f32(idepth)),
                                   _vp(_first(point, n)), _vp(_i32(target)), _vp(_i32(state)), _vp(_f32(idepth_hessian)), int(frames_to_marg), int(bool(only_empty)),
                                   _vp(fate), _vp(cand), _vp(counts))
    return fate, counts, cand


def run_standalone(extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -g -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once,
    returns its output; raises when it fails"""
    exe, _ = hb.build_program("winflag", SRC, "WFL_STANDALONE", extra_flags)
    return subprocess.check_output([exe], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/winflag_harness.py [g++ flags]: the sanitizer run of DESIGN §23
    import sys
    print(run_standalone(sys.argv[1:]), end="")
