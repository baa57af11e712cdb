"""Times DSO's initialiser on the device (include/eds_hip_init.h) at 640 x 480 with 5 levels: level 0 from the pixel selector at the
reference's density (0.03 W H, one recursion, th_factor 2), level 1 from a gradient threshold at the reference's 0.05 W H, the levels
above at full density; exact tables from eds_ini_make_nn.  A 10-frame sequence along a growing motion over a textured plane.

  set-up      eds_ini_set_first, the five eds_ini_set_points* and the five eds_ini_set_neighbours (the tables are made before, untimed
              and reported on their own: eds_ini_make_nn is a host search)
  trackFrame  per frame the call (host clock around it: upload, one launch, one wait) and the kernel (two events around the launch)
  serial      csrc/eds_init.hpp under g++ -O2 on the same input, one thread (tests/init_harness.py)

Also written: the points and the dependency-schedule depth of every level, and whether the device's results equal the serial ones.

    python tools/init_measure.py [--frames 10] [--out profiles/init_timing.json]
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
import init_harness as ih            # noqa: E402

init = importlib.import_module("slam-eds_amd.init")
select = importlib.import_module("slam-eds_amd.select")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_timing.json"))
    a = ap.parse_args()
    H, W, levels, cap = 480, 640, 5, 32768
    K = (520.0, 515.0, 322.3, 241.1)
    step = ((0.0015, -0.002, 0.003), (0.012, -0.007, 0.004))
    first = ic.frame_at(H, W, K, cc.se3((0, 0, 0), (0, 0, 0)))
    frames = [ic.frame_at(H, W, K, cc.se3(np.multiply(step[0], k), np.multiply(step[1], k))) for k in range(1, a.frames + 1)]
    colour = ic.pyramid_colour(first, levels)

    sel = select.Selector(H, W, table=np.random.default_rng(3).integers(0, 256, H * W).astype(np.uint8))
    sel.set_image(first)
    sel.potential = 3
    sel.make_maps(0.03 * W * H, 1, 2.0)
    status = [sel.map().astype(np.float32), ic.gradient_status(colour[1], 0.05 * W * H / colour[1].size)] + [np.ones_like(colour[l]) for l in range(2, levels)]
    uv = [ic.rect_points(s) for s in status]
    t0 = time.perf_counter()
    tables = [init.make_nn(uv[l], uv[l + 1] if l + 1 < levels else None) for l in range(levels)]
    make_nn_ms = (time.perf_counter() - t0) * 1e3

    def set_up(t, selector):
        t.setFirst(first)
        for l in range(levels):
            n = t.set_points_selected(selector) if (l == 0 and selector is not None) else t.set_points(l, status[l])
            assert n == len(uv[l]), (l, n, len(uv[l]))
        for l in range(levels):
            t.set_neighbours(l, *tables[l])

    dev = init.CoarseInitializer(H, W, levels, max_points_per_level=cap)
    dev.set_calib(*K)
    set_up(dev, sel)                                             # warm-up: the first launches load the code objects
    dev.trackFrame(frames[0])
    setup_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        set_up(dev, sel)
        setup_ms.append((time.perf_counter() - t0) * 1e3)
    call_ms, kernel_ms, results = [], [], []
    for f in frames:
        t0 = time.perf_counter()
        r = dev.trackFrame(f)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(dev.kernel_ms())
        results.append(r.copy())
        assert r["launches"] == 1 and r["waits"] == 1

    host = ih.HostInitializer(H, W, levels, max_points_per_level=cap)
    host.set_calib(*K)
    set_up(host, None)
    serial_ms, same = [], True
    for k, f in enumerate(frames):
        t0 = time.perf_counter()
        r = host.trackFrame(f)
        serial_ms.append((time.perf_counter() - t0) * 1e3)
        same = same and r.tobytes() == results[k].tobytes()
    for l in range(levels):
        same = same and dev.points(l).tobytes() == host.points(l).tobytes()

    out = dict(shape=[H, W, levels], frames=a.frames, points=[len(u) for u in uv], schedule_depth=[dev.schedule_depth(l) for l in range(levels)],
               make_nn_host_ms=round(make_nn_ms, 2), set_first_points_and_tables_ms=round(float(np.median(setup_ms)), 3),
               track_frame_call_ms=[round(v, 3) for v in call_ms], track_frame_kernel_ms=[round(v, 3) for v in kernel_ms],
               serial_gxx_ms=[round(v, 3) for v in serial_ms],
               median=dict(call_ms=round(float(np.median(call_ms)), 3), kernel_ms=round(float(np.median(kernel_ms)), 3),
                           serial_gxx_ms=round(float(np.median(serial_ms)), 3)),
               iterations=[int(r["n_decisions"]) for r in results], snapped=[int(r["snapped"]) for r in results],
               launches_per_frame=1, waits_per_frame=1, device_equals_serial=bool(same))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
