"""Cost of selecting a keyframe's candidate pixels (include/eds_hip_select.h) on one MI355X at the workload's own shape: 640 x 480,
density 1 500, the reference's random table, one recursion allowed, on a textured synthetic frame (seeded noise through synth.py's
Gaussian blur) that already lives in device memory.  The stage — eds_sel_set_image, eds_sel_make_maps, eds_imm_create_points_selected
with DSO's bounds — as host clocks (each call returns when its results are on the host): the median after a warm-up.  Alternating
with it in the same process, csrc/eds_pixsel.hpp (edspix::make_maps_serial, the same code on the CPU, tests/select_harness.py) on one
thread, every repetition compared bit for bit; and the route the device path replaces: download the image, the host selector,
eds_imm_create_points with the list.

--ramp times the frame on which EVERY pot cell is ambiguous (a pure horizontal ramp, min_grad_hist_add 0): the worst case of k_sel_scan.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_select.py --no-cpu` (never with counters).

    python tools/bench_select.py [--reps 7] [--no-cpu] [--ramp]
"""
import argparse
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
synth = importlib.import_module("slam-eds_amd.synth")
select = importlib.import_module("slam-eds_amd.select")
immature = importlib.import_module("slam-eds_amd.immature")
import select_harness as sh          # noqa: E402

H, W, DENSITY, RECURSIONS, MAX_POINTS = 480, 640, 1500.0, 1, 8000


def textured_frame(seed=2025):
    rng = np.random.default_rng(seed)
    img = synth.gaussian_blur(rng.standard_normal((H, W)), 9, 2.0) * 6.0 + 0.4 * synth.gaussian_blur(rng.standard_normal((H, W)), 3, 0.8)
    img = 128.0 + 90.0 * img / np.abs(img).max()
    return np.ascontiguousarray(np.clip(img, 0, 255), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--ramp", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_select needs a GPU: libeds_hip has no CPU fallback")
    prm = {}
    image = textured_frame()
    if a.ramp:
        image = np.tile(np.arange(W, dtype=np.float32) * np.float32(2.5) % np.float32(250.0), (H, 1))
        prm = dict(min_grad_hist_add=0.0)
    table = select.reference_pattern(H * W)
    rect = (3, 3, W - 5, H - 5)
    dev_image = capi.DeviceArray.from_numpy(image)
    s = select.Selector(H, W, table=table, **prm)
    ip = immature.ImmaturePoints(H, W, 1, MAX_POINTS, 1)
    ip.set_host_images(0, dev_image)
    ip2 = immature.ImmaturePoints(H, W, 1, MAX_POINTS, 1)
    ip2.set_host_images(0, dev_image)
    host = None if a.no_cpu else sh.HostSelector(H, W, table, **prm)

    t_img, t_maps, t_pts, t_stage, t_cpu, t_parent = [], [], [], [], [], []
    same, n_sub, n_pts, info = True, 0, 0, (0, 0)
    for rep in range(a.reps + 1):                              # the first repetition is the warm-up
        keep = rep > 0
        s.potential = 3
        t0 = time.perf_counter()
        s.set_image(dev_image)
        t1 = time.perf_counter()
        n_sub = s.make_maps(DENSITY, RECURSIONS)
        t2 = time.perf_counter()
        alive = ip.create_points_selected(0, s, rect)
        t3 = time.perf_counter()
        n_pts, info = len(alive), s.scan_info()
        if keep:
            for lst, v in zip((t_img, t_maps, t_pts, t_stage), (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                lst.append(v)
        if host is None:
            continue
        got_map, got_passes = s.map(), list(s.passes)
        host.potential = 3
        t0 = time.perf_counter()
        host.set_image(image)
        n_host = host.make_maps(DENSITY, RECURSIONS)
        t1 = time.perf_counter()
        same &= n_host == n_sub and np.array_equal(host.map(), got_map) and host.passes == got_passes
        host.potential = 3
        t0p = time.perf_counter()                               # the read-back route: the image comes down, the list goes up
        down = dev_image.numpy()
        host.set_image(down)
        host.make_maps(DENSITY, RECURSIONS)
        uv, typ = host.selection()
        k = (uv[:, 0] >= rect[0]) & (uv[:, 0] <= rect[2]) & (uv[:, 1] >= rect[1]) & (uv[:, 1] <= rect[3])
        alive2 = ip2.create_points(0, uv[k], typ[k])
        t1p = time.perf_counter()
        same &= np.array_equal(alive, alive2)
        if keep:
            t_cpu.append(t1 - t0)
            t_parent.append(t1p - t0p)
    med = lambda x: round(float(np.median(x)) * 1e3, 4)
    row = dict(H=H, W=W, density=DENSITY, recursions_left=RECURSIONS, frame="ramp" if a.ramp else "textured", reps=a.reps, passes=s.passes,
               num_have_sub=n_sub, points_created=n_pts, ambiguous_cells=info[0], potential_after=s.potential,
               gpu_set_image_ms=med(t_img), gpu_make_maps_ms=med(t_maps), gpu_create_points_selected_ms=med(t_pts), gpu_stage_ms=med(t_stage))
    if host is not None:
        row.update(cpu_set_image_make_maps_ms=med(t_cpu), read_back_route_stage_ms=med(t_parent), device_equals_cpu=bool(same))
    print(json.dumps(row), flush=True)
    for h in (s, ip, ip2):
        h.close()


if __name__ == "__main__":
    main()
