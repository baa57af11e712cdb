"""Times eds_ini_make_neighbours at the two levels of tests/test_inisetup_gpu.py's neighbour test: 6 497 points (the full 89 x 73
rectangle of a 96 x 80 level) below 700 points, and those 700 points as a top level.

  kernel_ms   eds_ini_get_neighbours_kernel_ms: the search kernel, two events around its launch
  call_ms     the whole eds_ini_make_neighbours on the host clock (read-backs, the host's tree build, uploads, the schedule)
  build_ms    the host's tree build alone — edsnn::build of csrc/eds_nntree.hpp under g++ (tests/inisetup_harness.py), the level's tree
              and the tree of the level above; absent for a library that does not build one

One untimed run first, then `--runs` timed ones; medians and extremes are written.  `--package DIR` loads slam-eds_amd from another
tree (a build of the parent commit), so that both libraries are timed on the same machine; `--label` names the entry of `--out`,
which is read, extended and written back.

    python tools/nn_pin_measure.py --label this_change [--package DIR] [--runs 5] [--out profiles/nn_pin_timing.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    return dict(median=round(float(np.median(ms)), 4), min=round(float(np.min(ms)), 4), max=round(float(np.max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-build-time", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_pin_timing.json"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.package), os.path.join(ROOT, "tests")]
    init = importlib.import_module("slam-eds_amd.init")

    H, W = 80, 96
    rng = np.random.default_rng(17)
    full = np.ones((H, W), np.float32)
    up = np.zeros((H // 2, W // 2), np.float32)
    ys, xs = np.mgrid[3:H // 2 - 4, 3:W // 2 - 4]
    pick = rng.choice(ys.size, size=700, replace=False)
    up[ys.ravel()[pick], xs.ravel()[pick]] = 1
    levels = {}
    with init.CoarseInitializer(H, W, 2, max_points_per_level=8192) as t:
        n = [t.set_points(0, full), t.set_points(1, up)]
        uv = [np.stack([t.points(l)["u"], t.points(l)["v"]], axis=1) for l in range(2)]
        for l in (1, 0):
            kernel, call = [], []
            for r in range(a.runs + 1):
                t0 = time.perf_counter()
                t.make_neighbours(l)
                ms = (time.perf_counter() - t0) * 1e3
                if r:
                    call.append(ms)
                    kernel.append(t.neighbours_kernel_ms())
            levels[f"{n[l]}_points"] = dict(level=l, n=n[l], n_up=n[1] if l == 0 else 0, kernel_ms=stats(kernel), call_ms=stats(call))
    if not a.no_build_time:
        import inisetup_harness as sh
        for l in (1, 0):
            build = []
            for r in range(a.runs + 1):
                t0 = time.perf_counter()
                sh.nn_build(uv[l])
                if l == 0:
                    sh.nn_build(uv[1])
                if r:
                    build.append((time.perf_counter() - t0) * 1e3)
            levels[f"{n[l]}_points"]["build_ms"] = stats(build)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out.setdefault("what", "eds_ini_make_neighbours at the levels of tests/test_inisetup_gpu.py's neighbour test; medians of "
                           f"{a.runs} runs after one untimed run, milliseconds; tools/nn_pin_measure.py")
    out[a.label] = levels
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({a.label: levels}))


if __name__ == "__main__":
    main()
