"""Times the depth-seeded creation of a keyframe's immature points (include/eds_hip_immdepth.h) on the device against the route a caller
had before it, in one process, the two legs alternating inside one loop so that whatever else the machine is doing falls on both.

  reference leg   Selector.selection() read back, the rectangle filter in numpy; the map on the host; edskd::build_tree and the walk
                  per pixel on one CPU thread (csrc/eds_immdepth.hpp under g++ -O2, tests/immdepth_harness.py); eds_imm_create_points
                  with its four uploaded arrays
  new leg         eds_imd_set_depth_map(on_device = 1) on the map where eds_map_window_depth_maps leaves it, then
                  eds_imd_create_points_selected

Sizes: 640 x 480, the selector at DSO's immature density (1 500) on a textured frame in device memory; maps of 2 000 and 4 096 points
(the device builds the tree) and 12 000 (beyond the capacity: the host builds it).  Every timed call ends with its own wait for the
stream, so a host clock around it is the call's time; the new leg's kernels are also timed with events (eds_imd_set_debug), in
repetitions of their own so that the events cost the host clocks nothing.  Warm-up repetitions first; medians, with the minimum and
maximum beside them.  Before anything is timed both legs' points and nearest neighbours are compared bit for bit.

    python tools/bench_immdepth.py [--reps 100] [--out profiles/immdepth_timing.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import immdepth_harness as dh          # noqa: E402
from bench_select import textured_frame          # noqa: E402

capi = importlib.import_module("slam-eds_amd.capi")
select = importlib.import_module("slam-eds_amd.select")
immature = importlib.import_module("slam-eds_amd.immature")
immdepth = importlib.import_module("slam-eds_amd.immdepth")
H, W, DENSITY, MAX_POINTS = 480, 640, 1500.0, 8000


def clock(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    return dict(median=float(np.median(times)), min=float(np.min(times)), max=float(np.max(times)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}") if a.dtype.kind == "f" else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "immdepth_timing.json"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_immdepth needs a GPU: nothing here is measured without one")
    hl = dh.load_harness()
    image = capi.DeviceArray.from_numpy(textured_frame())
    s = select.Selector(H, W, table=select.reference_pattern(H * W))
    s.set_image(image)
    s.make_maps(DENSITY, 1)
    rect = (3, 3, W - 5, H - 5)
    out = dict(unit="ms", reps=a.reps, warmup=a.warmup, image=[W, H], density=DENSITY, selected=int(s.num_selected), cases=[])
    for m in (2000, 4096, 12000):
        rng = np.random.default_rng(m)
        xy = np.stack([rng.uniform(0, W, m), rng.uniform(0, H, m)], axis=1)
        idp = rng.uniform(0.05, 2.0, m)
        d_xy, d_idp = capi.DeviceArray.from_numpy(xy), capi.DeviceArray.from_numpy(idp)
        new, ref = (immature.ImmaturePoints(H, W, 1, MAX_POINTS, 1) for _ in range(2))
        for ip in (new, ref):
            ip.set_host_images(0, image)
        d = immdepth.ImmatureDepth(new)
        res = {}

        def new_map():
            res["on_host"] = d.set_depth_map(d_xy, d_idp)

        def new_create():
            res["alive"], res["counts"] = d.create_points_selected(0, s, rect)

        def new_leg():
            new_map()
            new_create()

        def ref_select():
            uv, typ = s.selection()
            keep = (uv[:, 0] >= rect[0]) & (uv[:, 0] <= rect[2]) & (uv[:, 1] >= rect[1]) & (uv[:, 1] <= rect[3])
            res["uv"], res["typ"] = np.ascontiguousarray(uv[keep]), np.ascontiguousarray(typ[keep])

        def ref_tree():
            res["tree"] = dh.tree_of(hl, xy, idp)

        def ref_walk():
            res["nn"] = dh.nearest(hl, res["tree"], res["uv"])

        def ref_create():
            res["ref_alive"] = ref.create_points(0, res["uv"], res["typ"], res["nn"]["idepth"], res["nn"]["distance"])

        def ref_leg():
            ref_select()
            ref_tree()
            ref_walk()
            ref_create()
        # both routes give the same bits
        new_leg()
        ref_leg()
        assert np.array_equal(res["alive"], res["ref_alive"]) and new.num_points(0) == ref.num_points(0) == len(res["uv"])
        sa, sb = dict(new.get(0), **new.points(0)), dict(ref.get(0), **ref.points(0))
        assert all(np.array_equal(bits(sa[k]), bits(sb[k])) or np.array_equal(sa[k], sb[k], equal_nan=True) for k in sa)
        nn = d.nearest(0)
        assert all(np.array_equal(bits(nn[k]), bits(res["nn"][k])) for k in nn)
        calls = dict(new_leg=new_leg, reference_leg=ref_leg, new_set_depth_map=new_map, new_create_points_selected=new_create, reference_selection=ref_select,
                     reference_build_tree=ref_tree, reference_walk=ref_walk, reference_create_points=ref_create)
        for call in calls.values():
            for _ in range(a.warmup):
                call()
        times = {k: [] for k in calls}
        for _ in range(a.reps):                                   # the calls alternate
            for k, call in calls.items():
                times[k].append(clock(call))
        d.set_debug(timing=True)
        nn_ms, queue_ms = [], []
        for _ in range(a.reps):
            new_create()
            i = d.info()
            nn_ms.append(i["nn_kernel_ms"])
            queue_ms.append(i["queue_ms"])
        d.set_debug(timing=False)
        i = d.info()
        rec = dict(map_points=m, pixels=int(new.num_points(0)), good=int(res["counts"][0]), uninitialized=int(res["counts"][1]), tree_on_host=bool(res["on_host"]),
                   waits_per_create=int(i["waits"]))
        rec.update({k: stats(v) for k, v in times.items()})
        rec["nearest_kernel"] = stats(nn_ms)
        rec["create_queue_on_device"] = stats(queue_ms)
        rec["ratio_new_over_reference"] = rec["new_leg"]["median"] / rec["reference_leg"]["median"]
        out["cases"].append(rec)
        print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in rec.items()}))
        new.close()
        ref.close()
    s.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
