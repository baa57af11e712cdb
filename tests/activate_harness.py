"""ctypes side of tests/host_logic/activate_harness.cpp: csrc/eds_activate.hpp (namespace edsact, what the device kernels run) compiled
with g++ into a temporary directory where the tests run, and the stand-alone program of the same source with the cases dumped for it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import harness_build as hb
from immature_harness import POINT

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_logic", "activate_harness.cpp")
PARAM_ORDER = ("min_idepth_h_act", "gn_its_on_point_activation", "min_trace_quality", "max_trace_pixel_interval", "min_obs", "scale_idepth")
_INT = ("gn_its_on_point_activation", "min_obs")
_vp = C.c_void_p


def pack_params(prm):
    """eds_act_params / edsact::Params from the oracle's dict"""
    return b"".join(struct.pack("<i" if k in _INT else "<f", prm[k]) for k in PARAM_ORDER)


def to_struct(P, max_points):
    """the oracle's point set as max_points edsimm::Point"""
    n = len(P["u"])
    out = np.zeros(max_points, POINT)
    for k in ("color", "weights", "energyTH", "u", "v", "quality", "idepth_min", "idepth_max", "last_uv", "last_interval", "type", "status"):
        out[k][:n] = P[k]
    out["gradH"][:n] = P["gradH"]
    out["alive"][:n] = P["alive"]
    return out


def pack_points(Ps):
    """[n_hosts][max_points] points and the counts"""
    n = np.array([len(P["u"]) for P in Ps], np.int32)
    mp = max(1, int(n.max()))
    return np.stack([to_struct(P, mp) for P in Ps]), n, mp


_lib = None


def load_harness():
    global _lib
    if _lib is None:
        _lib = hb.load_library("activate", SRC)
        assert _lib.act_point_size() == POINT.itemsize == 128 and _lib.act_params_size() == len(pack_params({k: 0 for k in PARAM_ORDER}))
    return _lib


def _p(a):
    return a.ctypes.data_as(_vp)


def run_case(hl, c, prm, huber, pre=None):
    """make_map_serial, select_body with one thread and fit_serial over a case; the same outputs as activate_cases.oracle_run"""
    w1, h1 = c.W >> 1, c.H >> 1
    pts, n, mp = pack_points(c.P)
    K, T = np.ascontiguousarray(c.KRKi1, np.float32), np.ascontiguousarray(c.Kt1, np.float32)
    ah, ac = np.ascontiguousarray(c.active_host, np.int32), np.ascontiguousarray(c.active, np.float32)
    m = np.zeros(w1 * h1, np.uint8)
    hl.act_make_map(w1, h1, c.newest, _p(K), _p(T), len(ah), _p(ah), _p(ac), _p(m))
    seeded = np.zeros((h1, w1), np.float32)
    hl.act_map_values(_p(m), w1 * h1, _p(seeded))
    fate = np.zeros((c.F, mp), np.int32)
    counts = np.zeros(10, np.int32)
    fl = np.ascontiguousarray(c.flagged, np.uint8)
    pb = pack_params(prm)
    hl.act_select(_p(pts), mp, _p(n), c.newest, c.F, _p(K), _p(T), _p(fl), C.c_float(c.min_dist), pb, w1, h1, _p(m), _p(fate), _p(counts))
    selected = np.zeros((h1, w1), np.float32)
    hl.act_map_values(_p(m), w1 * h1, _p(selected))
    fates_sel = [fate[h, :n[h]].copy() for h in range(c.F)]
    colors = np.ascontiguousarray(np.stack(c.images), np.float32)
    pre = np.ascontiguousarray(c.pre if pre is None else pre, np.float32)
    fit = np.zeros((c.F, mp, 4), np.float32)
    rs, re = np.zeros((c.F, mp, c.F), np.int32), np.zeros((c.F, mp, c.F), np.float32)
    fx, fy, cx, cy = (C.c_float(x) for x in c.K4)
    hl.act_optimize(_p(pts), mp, _p(n), c.F, _p(pre), _p(colors), c.H, c.W, fx, fy, cx, cy, pb, C.c_float(huber), _p(fate), _p(fit), _p(rs), _p(re))
    results = [dict(idepth=fit[h, :n[h], 0], energy=fit[h, :n[h], 1], hdd=fit[h, :n[h], 2], bd=fit[h, :n[h], 3], res_state=rs[h, :n[h]],
                    res_energy=re[h, :n[h]]) for h in range(c.F)]
    return dict(map_seeded=seeded, map_selected=selected, fates_selected=fates_sel, fates=[fate[h, :n[h]] for h in range(c.F)], results=results,
                alive=[pts[h]["alive"][:n[h]].astype(bool) for h in range(c.F)], counts=counts)


def dump_cases(path, cases, prm_of, huber):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            pts, n, mp = pack_points(c.P)
            f.write(struct.pack("<6i", c.H, c.W, c.F, mp, c.newest, len(c.active_host)))
            f.write(pack_params(prm_of(c)))
            f.write(struct.pack("<f4ff", huber, *c.K4, c.min_dist))
            f.write(n.tobytes())
            f.write(pts.tobytes())
            f.write(np.ascontiguousarray(np.stack(c.images), np.float32).tobytes())
            f.write(np.ascontiguousarray(c.KRKi1, np.float32).tobytes())
            f.write(np.ascontiguousarray(c.Kt1, np.float32).tobytes())
            f.write(np.ascontiguousarray(c.active_host, np.int32).tobytes())
            f.write(np.ascontiguousarray(c.active, np.float32).tobytes())
            f.write(np.ascontiguousarray(c.flagged, np.uint8).tobytes())
            f.write(np.ascontiguousarray(c.pre, np.float32).tobytes())


def run_standalone(cases, prm_of, huber, extra_flags=()):
    """builds the stand-alone program (extra_flags: e.g. -fsanitize=address,undefined -fno-sanitize-recover=all), runs it once over
    `cases` plus its own hostile inputs, returns its output; raises when it fails"""
    exe, data = hb.build_program("activate", SRC, "ACT_STANDALONE", extra_flags)
    dump_cases(data, cases, prm_of, huber)
    return subprocess.check_output([exe, data], text=True, stderr=subprocess.STDOUT)


if __name__ == "__main__":          # python tests/activate_harness.py [g++ flags]: the sanitizer run of DESIGN §19
    import sys
    sys.path.insert(0, HERE)
    import activate_cases as ac
    import np_activate_oracle as ao
    import np_immature_oracle as no
    print(run_standalone(list(ac.cases().values()), lambda c: ao.params(**c.act_prm), float(no.params()["huber_th"]), sys.argv[1:]), end="")
