"""Cost of DSO's coarse image tracker (include/eds_hip_coarse.h) on one MI355X at 640 x 480 with 5 levels and 2 000 active points x 7
keyframes as contributions, for 1, 8 and 32 tries (initial guesses scattered around the true motion).  Per row: the per-level list
sizes, the iterations and accepts per level of the first try, and the median host-clock time around eds_ct_set_ref, eds_ct_set_new and
eds_ct_track (each returns when its results are on the host) after a warm-up; alternating with the device in the same process,
edsct::track_serial (csrc/eds_coarse.hpp, the same code on the CPU, tests/coarse_harness.py) on one thread and with the tries spread
over 16.  The device's results are compared with the CPU's once per row, bit for bit.

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_coarse.py --tries 8 --no-cpu` (never with counters).

    python tools/bench_coarse.py [--tries 1 8 32] [--reps 7] [--no-cpu]
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
coarse = importlib.import_module("slam-eds_amd.coarse")
import coarse_cases as cc            # noqa: E402
import coarse_harness as ch          # noqa: E402
import np_coarse_oracle as no        # noqa: E402

H, W, LEVELS, K4, N = 480, 640, 5, (535.0, 530.0, 322.5, 238.25), 7 * 2000
THREADS = 16


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=7)        # DESIGN 16's table is the default
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_coarse needs a GPU: libeds_hip has no CPU fallback")
    c = cc.make(2025, H, W, LEVELS, K4, N, ((0.003, -0.004, 0.006), (0.02, -0.01, 0.006)), gain=(0.03, 3.0), dup=0.05)
    rng = np.random.default_rng(5)
    pool = ThreadPoolExecutor(THREADS)
    t = coarse.CoarseTracker(H, W, LEVELS, max_points=N, max_tries=max(a.tries))
    t.set_calib(*c.K)
    host = None if a.no_cpu else ch.open_case(c)
    for B in a.tries:
        tries = np.stack([cc.IDENT] + [cc.se3(0.004 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)) for _ in range(B - 1)])
        affs = np.zeros((B, 2))
        t.set_ref(c.ref, c.cp, c.hdif)
        t.set_new(c.new)
        r = t.track(tries, affs)                                                       # warm-up
        row = dict(tries=B, H=H, W=W, levels=LEVELS, contributions=N, reps=a.reps, pc_n=t.pc_n.tolist(),
                   iterations_try0=r["iterations"][0].tolist(), accepts_try0=r["accepts"][0].tolist(),
                   iterations_all=int(r["iterations"].sum()), ok=int(r["ok"].sum()),
                   pose_error_try0=float(np.abs(r["T"][0] - c.T_true).max()))
        g_track, c1, c16 = [], [], []
        for _ in range(a.reps):                                                        # alternating
            t0 = time.perf_counter()
            r = t.track(tries, affs)
            g_track.append(time.perf_counter() - t0)
            if a.no_cpu:
                continue
            t0 = time.perf_counter()
            rc = host.track(tries, affs)
            c1.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            list(pool.map(lambda k: host.track(tries[k], affs[k]), range(B)))
            c16.append(time.perf_counter() - t0)
        g = float(np.median(g_track))
        row.update(set_ref_ms=median_ms(lambda: t.set_ref(c.ref, c.cp, c.hdif), a.reps), set_new_ms=median_ms(lambda: t.set_new(c.new), a.reps),
                   track_ms=round(g * 1e3, 4), track_ms_per_try=round(g * 1e3 / B, 4))
        if not a.no_cpu:
            row.update(device_equals_cpu=all(no.same_bits(r[f], rc[f]) for f in r.dtype.names), cpu_1_thread_ms=round(float(np.median(c1)) * 1e3, 3),
                       cpu_16_threads_ms=round(float(np.median(c16)) * 1e3, 3), cpu_1_over_gpu=round(float(np.median(c1)) / g, 2),
                       cpu_16_over_gpu=round(float(np.median(c16)) / g, 2))
        print(json.dumps(row), flush=True)
    t.close()


if __name__ == "__main__":
    main()
