"""Cost of activating immature points (include/eds_hip_activate.h) on one MI355X: 640 x 480, F = 7 window frames, 2 000 immature points
per host with the intervals four traces leave, 2 000 active points.  Per call — eds_act_make_distance_map, eds_act_select,
eds_act_optimize — the median host-clock time (each returns when its results are on the host) after a warm-up, and, alternating with
it in the same process, csrc/eds_activate.hpp (edsact::, the same code on the CPU, tests/activate_harness.py) on one thread; every
repetition starts from the same traced points and is compared with the CPU's bit for bit.  Then the whole stage both ways: on the
device (the three calls, eds_act_get_activated, the window's tables set), and by the only route there was before (eds_imm_get and
eds_imm_get_points for every host, edsact:: on the host with the frames' gradients already there, the tables set).

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_activate.py --no-cpu` (never with counters).

    python tools/bench_activate.py [--reps 7] [--no-cpu] [--min-dist 2.0]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
capi = importlib.import_module("slam-eds_amd.capi")
immature = importlib.import_module("slam-eds_amd.immature")
activate = importlib.import_module("slam-eds_amd.activate")
window = importlib.import_module("slam-eds_amd.window")
import activate_cases as ac          # noqa: E402
import activate_harness as ah        # noqa: E402
import immature_cases as ic          # noqa: E402
import np_activate_oracle as ao      # noqa: E402
import np_immature_oracle as no      # noqa: E402

H, W, F, N, N_ACTIVE, K4 = 480, 640, 7, 2000, 2000, (535.0, 530.0, 322.5, 238.25)


def scene():
    sc = ic.Scene(2025, H, W, K4)
    rng = sc.rng
    poses = [(ic.rot(*rng.uniform(-0.01, 0.01, 2), rng.uniform(-0.03, 0.03)), np.append(rng.uniform(-0.03, 0.03, 2), rng.uniform(-0.01, 0.01))) for _ in range(F)]
    images = [sc.render(R, p) for R, p in poses]
    uv = [np.stack([rng.integers(8, W - 8, N), rng.integers(8, H - 8, N)], axis=1).astype(np.int32) for _ in poses]
    targets, steps = [], []
    for k in range(4):
        Rt, pt = ic.rot(0.002 * k, -0.003 * k, 0.004 * k), np.array([0.03, 0.004, 0.002]) * (k + 1)
        targets.append(sc.render(Rt, pt))
        steps.append([ic.precalc32(K4, Rt.T @ R, Rt.T @ (p - pt)) for R, p in poses])
    newest = F - 1
    K1, T1 = zip(*[ac.distance_precalc(K4, *ac.relative(poses, h, newest)) for h in range(F)])
    per = N_ACTIVE // F
    active_host = np.repeat(np.arange(F, dtype=np.int32), per)
    active = np.stack([rng.uniform(3, W - 3, len(active_host)), rng.uniform(3, H - 3, len(active_host)), 0.5 * (1 + 0.05 * rng.standard_normal(len(active_host)))],
                      axis=1).astype(np.float32)
    return dict(poses=poses, images=np.stack(images), uv=uv, targets=np.stack(targets), steps=steps, newest=newest, KRKi1=np.stack(K1), Kt1=np.stack(T1),
                active_host=active_host, active=active, pre=ac.precalc(poses))


def download(h):
    """the parent commit's read-back: every host's intervals and constructor outputs, as edsimm::Point"""
    pts = np.zeros((F, N), ah.POINT)
    for i in range(F):
        g, p = h.get(i), h.points(i)
        o = pts[i]
        o["idepth_min"], o["idepth_max"], o["quality"], o["status"] = g["idepth_min"], g["idepth_max"], g["quality"], g["lastTraceStatus"]
        o["last_uv"], o["last_interval"] = g["lastTraceUV"], g["lastTracePixelInterval"]
        o["color"], o["weights"], o["gradH"], o["energyTH"], o["alive"] = p["color"], p["weights"], p["gradH"].reshape(-1, 4), p["energyTH"], p["alive"]
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--min-dist", type=float, default=2.0)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_activate needs a GPU: libeds_hip has no CPU fallback")
    s = scene()
    hl = ah.load_harness()
    prm = ao.params()
    pb = ah.pack_params(prm)
    huber = float(no.params()["huber_th"])
    w1, h1 = W >> 1, H >> 1
    n = np.full(F, N, np.int32)
    flagged = np.zeros(F, np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    grads = np.zeros((F, H, W, 2), np.float32)
    hl.act_gradients(p(s["images"]), F, H, W, p(grads))
    fx, fy, cx, cy = (C.c_float(x) for x in K4)

    h = immature.ImmaturePoints(H, W, F, N, 4)
    h.set_host_images(0, s["images"])
    h.set_target_images(0, s["targets"])
    act = activate.Activation(h, *K4)
    win = window.Window(H, W, F, max_points=F * N, max_residuals=F * N * (F - 1))
    win.set_calib(*K4)
    win.set_frames(0, s["images"])
    args = [tuple(np.stack([st[j] for st in step]) for j in range(3)) for step in s["steps"]]

    def prepare():
        for i in range(F):
            h.create_points(i, s["uv"][i])
        for k in range(4):
            h.trace(0, [k] * F, *args[k])

    def set_tables(points, residuals):
        win.set_points(points["host"], points["uv"], points["color"], points["weights"], points["idepth_scaled"], points["idepth_zero_scaled"])
        win.set_residuals(residuals["point"], residuals["target"], residuals["state"], residuals["energy"])

    def cpu(pts, times=None):
        uvf = [u.astype(np.float32) for u in s["uv"]]
        for i in range(F):
            pts[i]["u"], pts[i]["v"], pts[i]["type"] = uvf[i][:, 0], uvf[i][:, 1], 1.0
        m = np.zeros(w1 * h1, np.uint8)
        fate, counts = np.zeros((F, N), np.int32), np.zeros(10, np.int32)
        fit, rs, re = np.zeros((F, N, 4), np.float32), np.zeros((F, N, F), np.int32), np.zeros((F, N, F), np.float32)
        t0 = time.perf_counter()
        hl.act_make_map(w1, h1, s["newest"], p(s["KRKi1"]), p(s["Kt1"]), len(s["active_host"]), p(s["active_host"]), p(s["active"]), p(m))
        t1 = time.perf_counter()
        hl.act_select(p(pts), N, p(n), s["newest"], F, p(s["KRKi1"]), p(s["Kt1"]), p(flagged), C.c_float(a.min_dist), pb, w1, h1, p(m), p(fate), p(counts))
        t2 = time.perf_counter()
        hl.act_optimize_g(p(pts), N, p(n), F, p(s["pre"]), p(s["images"]), p(grads), H, W, fx, fy, cx, cy, pb, C.c_float(huber), p(fate), p(fit), p(rs), p(re))
        t3 = time.perf_counter()
        if times is not None:
            for k, v in zip(("map", "select", "optimize"), (t1 - t0, t2 - t1, t3 - t2)):
                times[k].append(v)
        mv = np.zeros((h1, w1), np.float32)
        hl.act_map_values(p(m), w1 * h1, p(mv))
        return mv, fate, fit, rs, re

    def tables_from_cpu(pts, fate, fit, rs):
        hh, ii = np.nonzero(fate == ao.ACTIVATED)
        sel = pts[hh, ii]
        points = dict(host=hh.astype(np.int32), uv=np.stack([sel["u"], sel["v"]], axis=1), color=sel["color"], weights=sel["weights"],
                      idepth_scaled=fit[hh, ii, 0], idepth_zero_scaled=fit[hh, ii, 0])
        pi, tt = np.nonzero(rs[hh, ii] == ao.ST_IN)
        return points, dict(point=pi.astype(np.int32), target=tt.astype(np.int32), state=np.zeros(len(pi), np.int32), energy=np.zeros(len(pi), np.float32))

    g = dict(map=[], select=[], optimize=[], stage=[])
    c = dict(map=[], select=[], optimize=[])
    parent = []
    same = True
    counts = None
    for rep in range(a.reps + 1):                              # the first repetition is the warm-up
        keep = rep > 0
        prepare()
        t0 = time.perf_counter()
        act.make_distance_map(s["newest"], s["KRKi1"], s["Kt1"], s["active_host"], s["active"])
        t1 = time.perf_counter()
        act.select(s["newest"], s["KRKi1"], s["Kt1"], flagged, a.min_dist)
        t2 = time.perf_counter()
        counts = act.optimize(s["pre"])
        t3 = time.perf_counter()
        set_tables(*act.window_tables())
        t4 = time.perf_counter()
        if keep:
            for k, v in zip(("map", "select", "optimize", "stage"), (t1 - t0, t2 - t1, t3 - t2, t4 - t0)):
                g[k].append(v)
        if a.no_cpu:
            continue
        got_map = act.distance_map()
        got = [act.get(i) for i in range(F)]
        prepare()
        t0 = time.perf_counter()
        pts = download(h)
        mv, fate, fit, rs, re = cpu(pts, c if keep else None)
        set_tables(*tables_from_cpu(pts, fate, fit, rs))
        if keep:
            parent.append(time.perf_counter() - t0)
        same &= bool(no.same_bits(got_map, mv).all())
        for i in range(F):
            same &= bool((got[i]["fate"] == fate[i]).all() and no.same_bits(got[i]["res_energy"], re[i]).all() and (got[i]["res_state"] == rs[i]).all())
            for j, k in enumerate(("idepth", "energy", "hdd", "bd")):
                same &= bool(no.same_bits(got[i][k], fit[i, :, j]).all())
    med = lambda x: round(float(np.median(x)) * 1e3, 4)
    row = dict(H=H, W=W, frames=F, points_per_host=N, active_points=len(s["active_host"]), min_act_dist=a.min_dist, reps=a.reps,
               fates={activate.FATE_NAMES[i]: int(v) for i, v in enumerate(counts) if v},
               gpu_make_distance_map_ms=med(g["map"]), gpu_select_ms=med(g["select"]), gpu_optimize_ms=med(g["optimize"]), gpu_stage_ms=med(g["stage"]))
    if not a.no_cpu:
        row.update(cpu_make_distance_map_ms=med(c["map"]), cpu_select_ms=med(c["select"]), cpu_optimize_ms=med(c["optimize"]),
                   parent_route_stage_ms=med(parent), device_equals_cpu=same)
    print(json.dumps(row), flush=True)
    win.close()
    h.close()


if __name__ == "__main__":
    main()
