"""Cost of the window optimiser's inner loop (include/eds_hip_window.h) on one MI355X at 640 x 480 with F = 7 frames, 2 000 points per
host frame and a residual towards every other frame.  Per call (eds_win_set_idepths, eds_win_linearize, eds_win_apply,
eds_win_point_hessians, eds_win_accumulate — each returns when its results are on the device or the host): the median of `reps`
host-clock times after a warm-up, alternating in the same process with edswin:: (csrc/eds_window.hpp, the same code on the CPU,
tests/window_harness.py) on one thread and, for the three per-residual / per-point stages, with the points sliced by 50 over a pool of
16 threads (accumulate_serial is one loop: one thread only).  Every row's results are compared with the device's bit for bit.

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_window.py --no-cpu` (never with counters).

    python tools/bench_window.py [--reps 7] [--no-cpu]
"""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
capi = importlib.import_module("slam-eds_amd.capi")
window = importlib.import_module("slam-eds_amd.window")
import window_cases as wc            # noqa: E402
import window_harness as wh          # noqa: E402

H, W, F, PER_HOST, K4, THREADS, GRAIN = 480, 640, 7, 2000, (535.0, 530.0, 322.5, 238.25), 16, 50
STAGES = ("set_idepths", "linearize", "apply", "point_hessians", "accumulate")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def one_round(w, c, ids, pool=None):
    """the loop's calls in order; returns (seconds per stage, everything the calls returned)"""
    t, shift = {}, bool(c.shift)
    t["set_idepths"], _ = timed(lambda: w.set_idepths(ids))
    if pool is None:
        t["linearize"], lin = timed(lambda: w.linearize(c.F, c.precalc, c.th))
        t["apply"], _ = timed(lambda: w.apply(True))
        t["point_hessians"], nres = timed(lambda: w.point_hessians(c.prior, c.delta, c.lf, shift))
    else:
        t["linearize"], lin = timed(lambda: w.linearize_pool(pool, c.F, c.precalc, c.th, GRAIN))
        t["apply"], _ = timed(lambda: w.apply_pool(pool, True, GRAIN))
        t["point_hessians"], nres = timed(lambda: w.point_hessians_pool(pool, c.prior, c.delta, c.lf, shift, GRAIN))
    t["accumulate"], acc = timed(lambda: w.accumulate(c.F, c.adH, c.adT, c.prior, c.delta, c.lf, shift))
    return t, dict(acc, energy=np.float64(lin[0]), counts=lin[1], nres_points=np.int32(nres))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        u = f"u{a.dtype.itemsize}"
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)        # DESIGN 17's table is the default
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_window needs a GPU: libeds_hip has no CPU fallback")
    c = wc.make(2026, F, [PER_HOST] * F, shift=1, shape=(H, W), K=K4)
    n, m = len(c.host), len(c.point)
    dev = wh.open_case(c, cls=lambda H_, W_, F_: window.Window(H_, W_, F_, max_points=n, max_residuals=m))
    sides = {"device": (dev, None)}
    pool = ThreadPoolExecutor(THREADS)
    if not a.no_cpu:
        sides["cpu_1_thread"] = (wh.open_case(c), None)
        sides["cpu_16_threads"] = (wh.open_case(c), pool)
    for w, p in sides.values():
        one_round(w, c, c.ids, p)                             # warm-up
    times = {k: {s: [] for s in STAGES} for k in sides}
    equal = {k: True for k in sides if k != "device"}
    for rep in range(a.reps):                                 # alternating; the idepths change every round, as after a step
        ids = c.ids2 if rep % 2 == 0 else c.ids
        out = {}
        for k, (w, p) in sides.items():
            t, out[k] = one_round(w, c, ids, p)
            for s in STAGES:
                times[k][s].append(t[s])
        for k in equal:
            equal[k] = equal[k] and all(same(out["device"][f], out[k][f]) for f in out["device"])
    for k in equal:                                           # and everything else a caller can read
        rd, rc, pd, pc = dev.residuals(), sides[k][0].residuals(), dev.points(), sides[k][0].points()
        equal[k] = equal[k] and all(same(rd[f], rc[f]) for f in rd) and all(same(pd[f], pc[f]) for f in pd)
    med = {k: {s: float(np.median(v)) for s, v in ts.items()} for k, ts in times.items()}
    row = dict(H=H, W=W, F=F, points=n, residuals=m, reps=a.reps, counts=out["device"]["counts"].tolist(), nres=int(out["device"]["nres"]),
               accumulator_words=int(len(out["device"]["acc"])), residuals_per_s=round(m / med["device"]["linearize"]))
    for k in sides:
        for s in STAGES:
            row[f"{k}_{s}_ms"] = round(med[k][s] * 1e3, 4)
        if k != "device":
            row[f"{k}_equals_device"] = bool(equal[k])
            row[f"{k}_over_device_loop"] = round(sum(med[k].values()) / sum(med["device"].values()), 2)
    print(json.dumps(row), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
