"""Times the rest of setFirst on the device (include/eds_hip_inisetup.h) at 640 x 480 with 5 levels, the selector's points at the
reference densities {0.03, 0.05, 0.15, 0.5, 1}.

  setup_levels        eds_ini_setup_levels as a whole (host clock around the call; the sparsity is put back to 5 before every repetition)
  make_pixel_status   each eds_ini_make_pixel_status of levels 1 .. 4 in the reference's order, with its passes
  make_neighbours     each eds_ini_make_neighbours: the call, and the search kernel (two events around its launch)
  before              on the same machine and the same points, what a caller had before: eds_ini_make_nn (one host thread) and
                      eds_ini_set_neighbours per level, each on its own

Every timed thing runs once untimed first (the first launches load the code objects), then `--reps` times; the medians and the
extremes are written.  Also written: the points per level and whether the device's tables equal eds_ini_make_nn's.

    python tools/inisetup_measure.py [--reps 7] [--out profiles/inisetup_timing.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import coarse_cases as cc            # noqa: E402
import init_cases as ic              # noqa: E402

init = importlib.import_module("slam-eds_amd.init")
select = importlib.import_module("slam-eds_amd.select")

DENSITIES = np.float32([0.03, 0.05, 0.15, 0.5, 1.0])


def stats(ms):
    return dict(median=round(float(np.median(ms)), 4), min=round(float(np.min(ms)), 4), max=round(float(np.max(ms)), 4))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inisetup_timing.json"))
    a = ap.parse_args()
    H, W, levels, cap = 480, 640, 5, 32768
    K = (520.0, 515.0, 322.3, 241.1)
    first = ic.frame_at(H, W, K, cc.se3((0, 0, 0), (0, 0, 0)))
    density = [float(np.float32(np.float32(d * np.float32(W)) * np.float32(H))) for d in DENSITIES]

    sel = select.Selector(H, W, table=np.random.default_rng(3).integers(0, 256, H * W).astype(np.uint8))
    sel.set_image(first)
    dev = init.CoarseInitializer(H, W, levels, max_points_per_level=cap)
    dev.set_calib(*K)
    dev.setFirst(first)

    whole = []
    for rep in range(a.reps + 1):
        dev.sparsity = 5
        ms, n = timed(lambda: dev.setup_levels(sel))
        if rep:
            whole.append(ms)
    points = [int(k) for k in n]

    status_ms, passes = {l: [] for l in range(1, levels)}, {}
    for rep in range(a.reps + 1):
        dev.sparsity = 5
        for l in range(1, levels):
            ms, (n_good, p) = timed(lambda: dev.make_pixel_status(l, density[l]))
            passes[l] = p
            if rep:
                status_ms[l].append(ms)
    for l in range(1, levels):                                               # the maps are the same ones: the points stay
        assert dev.set_points_status(l) == points[l], (l, points)

    call_ms, kernel_ms = {l: [] for l in range(levels)}, {l: [] for l in range(levels)}
    for rep in range(a.reps + 1):
        for l in range(levels - 1, -1, -1):
            ms, _ = timed(lambda: dev.make_neighbours(l))
            if rep:
                call_ms[l].append(ms)
                kernel_ms[l].append(dev.neighbours_kernel_ms())

    uv = [np.stack([dev.points(l)["u"], dev.points(l)["v"]], axis=1) for l in range(levels)]
    made = [dev.neighbours(l) for l in range(levels)]
    depth = [dev.schedule_depth(l) for l in range(levels)]
    host_nn_ms, set_nb_ms, same = {l: [] for l in range(levels)}, {l: [] for l in range(levels)}, True
    for rep in range(min(a.reps, 3) + 1):
        for l in range(levels - 1, -1, -1):
            ms, (nb, par) = timed(lambda: init.make_nn(uv[l], uv[l + 1] if l + 1 < levels else None))
            ms2, _ = timed(lambda: dev.set_neighbours(l, nb, par))
            same = same and nb.tobytes() == made[l][0].tobytes() and (par is None or par.tobytes() == made[l][1].tobytes())
            if rep:
                host_nn_ms[l].append(ms)
                set_nb_ms[l].append(ms2)
    same = same and depth == [dev.schedule_depth(l) for l in range(levels)]

    per_level = []
    for l in range(levels):
        before = float(np.median(host_nn_ms[l]) + np.median(set_nb_ms[l]))
        per_level.append(dict(level=l, points=points[l], schedule_depth=depth[l],
                              make_pixel_status_ms=stats(status_ms[l]) if l else None, passes=passes.get(l),
                              make_neighbours_call_ms=stats(call_ms[l]), make_neighbours_kernel_ms=stats(kernel_ms[l]),
                              before_make_nn_host_ms=stats(host_nn_ms[l]), before_set_neighbours_ms=stats(set_nb_ms[l]),
                              before_ms=round(before, 4), not_slower=bool(np.median(call_ms[l]) <= before)))
    out = dict(shape=[H, W, levels], reps=a.reps, densities=[float(d) for d in DENSITIES], points=points, setup_levels_ms=stats(whole),
               levels=per_level, device_tables_equal_make_nn=bool(same), not_slower_on_every_level=all(p["not_slower"] for p in per_level))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
