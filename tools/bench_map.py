"""Times the keyframe hand-over of include/eds_hip_map.h on the device against the route a caller had before it, in one process, the two
legs alternating inside one loop so that whatever else the machine is doing falls on both.

  reference leg   read uv (eds_wed_get) and idepth_scaled (eds_wsv_get) back, run edsmap::'s serial restatement on the host
                  (csrc/eds_map.hpp under g++ -O2, one thread), eds_kfs_build_keyframes_dev with EDS_KFS_DEPTH_HOST
  new leg         eds_map_window_depth_maps(on_device = 1), eds_kfs_build_keyframes_dev with EDS_KFS_DEPTH_DEVICE

Both legs take the new keyframes' images from device memory and ask for no point vectors back, so the difference is the map's path
alone.  The map stage of either leg is also timed without the keyframe build, and eds_map_window_cloud alone with both fans, into host
memory and into device memory.  Sizes: a full DSO window of 7 frames x 2 000 points, and 7 x 300; 1 and 4 destination keyframes of
640 x 480.  Every timed call ends with its own wait for the stream, so a host clock around it is the call's time.  Warm-up repetitions
first; medians, with the minimum and maximum beside them.  Before anything is timed both legs' maps are compared bit for bit, and the
slots they leave are compared.

    python tools/bench_map.py [--reps 200] [--out profiles/map_timing.json]
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import kdbuild_cases as kc          # noqa: E402
import map_cases as mc              # noqa: E402
import map_harness as mh            # noqa: E402
import np_map_oracle as mo          # noqa: E402

capi = importlib.import_module("slam-eds_amd.capi")
window = importlib.import_module("slam-eds_amd.window")
winsolve = importlib.import_module("slam-eds_amd.winsolve")
winedit = importlib.import_module("slam-eds_amd.winedit")
mp = importlib.import_module("slam-eds_amd.map")
H, W, F = 480, 640, 7
SELECT = dict(method=capi.KF_MAX, num_points=2000)       # the new keyframes' own points: the strongest gradients, 2 000 of them


def clock(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    return dict(median=float(np.median(times)), min=float(np.min(times)), max=float(np.max(times)))


def scene(per_frame, count, seed):
    rng = np.random.default_rng(seed)
    n = F * per_frame
    K = np.array([0.78 * W, 0.78 * W, 0.5 * W - 0.5, 0.5 * H - 0.5])
    c = dict(host=np.repeat(np.arange(F), per_frame).astype(np.int32), ids=rng.uniform(0.3, 2.0, n).astype(np.float32),
             uv=np.stack([rng.uniform(3, W - 4, n), rng.uniform(3, H - 4, n)], axis=1).astype(np.float32), calib=K.astype(np.float32),
             T_w_c=np.stack([mc.random_pose(rng, 0.05, 0.15) for _ in range(F)]), mask=(1 << F) - 1)
    c["T_dst_w"] = np.stack([mc.inverse(mc.random_pose(rng, 0.05, 0.15)) for _ in range(count)])
    c["K_dst"] = np.stack([K * [1.0 + 0.01 * b, 1.0 - 0.01 * b, 1.0, 1.0] for b in range(count)])
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_timing.json"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_map needs a GPU: nothing here is measured without one")
    out = dict(unit="ms", reps=a.reps, warmup=a.warmup, frames=F, dst=[W, H], images="device memory, float32", vectors=False, keyframe_select="KF_MAX, num_points 2000", cases=[])
    HL = mh.load_harness()
    for per_frame in (2000, 300):
        for count in (1, 4):
            c = scene(per_frame, count, 7 * per_frame + count)
            n = len(c["host"])
            w = window.Window(H, W, 8, max_points=n, max_residuals=1)
            w.set_calib(*[float(v) for v in c["calib"]])
            w.set_points(c["host"], c["uv"], np.zeros((n, 8), np.float32), np.ones((n, 8), np.float32), c["ids"], c["ids"])
            sv, ed = winsolve.WindowSolver(w), winedit.WindowEdit(w)
            eye = np.tile(np.eye(8), (F * F, 1, 1))
            sv.set_state(F, eye, eye, np.zeros((F, 8)), np.ones((F, 8)), np.zeros((F, 8)), np.ones(4), np.zeros(4))      # eds_wsv_get wants a state
            cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4)
            trk = [capi.Handle(cfg, count, 4096, H, W) for _ in range(2)]
            imgs = capi.DeviceArray.from_numpy(np.stack([kc.image(40 + b, H, W) for b in range(count)]))
            T, Td, Kd, cal = (np.ascontiguousarray(c[k]) for k in ("T_w_c", "T_dst_w", "K_dst", "calib"))
            # the reference leg's buffers, allocated once
            host, uv, ids = np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
            xy, idp, cnt = np.zeros((count, n, 2)), np.zeros((count, n)), np.zeros(count, np.int32)
            wed_out, wsv_out = winedit.Out(host=host.ctypes.data, uv=uv.ctypes.data), winsolve.Out(idepth_scaled=ids.ctypes.data)
            LW, LS = winedit._lib(), winsolve._lib()
            maps = {}

            def ref_map():
                capi._check(LW.eds_wed_get(w._h, C.byref(wed_out)))
                capi._check(LS.eds_wsv_get(w._h, C.byref(wsv_out)))
                assert HL.map_window_depth_maps(n, capi.vp(host), capi.vp(uv), capi.vp(ids), capi.vp(cal), F, c["mask"], capi.vp(T), count, capi.vp(Td),
                                                capi.vp(Kd), H, W, n, capi.vp(xy), capi.vp(idp), None, capi.vp(cnt)) == 0

            def ref_leg():
                ref_map()
                return trk[0].build_keyframes(imgs, Kd, depth=[xy[b, :cnt[b]] for b in range(count)], depth_idp=[idp[b, :cnt[b]] for b in range(count)],
                                              vectors=False, **SELECT)

            # the new leg's buffers, allocated once as well: the caller's device memory
            d_xy, d_idp, d_n = capi.DeviceArray((count, n, 2), np.float64), capi.DeviceArray((count, n), np.float64), np.zeros(count, np.int32)
            maps["m"] = dict(depth_xy=d_xy, depth_idp=d_idp, n=d_n)
            LM = mp._lib()

            def new_map():
                capi._check(LM.eds_map_window_depth_maps(w._h, F, c["mask"], capi.vp(T), count, capi.vp(Td), capi.vp(Kd), H, W, n, C.c_void_p(d_xy.ptr),
                                                         C.c_void_p(d_idp.ptr), None, 1, capi.vp(d_n)))

            def new_leg():
                new_map()
                m = maps["m"]
                return trk[1].build_keyframes(imgs, Kd, depth=m["depth_xy"], depth_idp=m["depth_idp"], depth_n=m["n"], vectors=False, **SELECT)
            # the two legs give the same maps and leave the same slots
            ra, rb = ref_leg(), new_leg()
            m = maps["m"]
            assert m["n"].tolist() == cnt.tolist() and all(0 < k < n for k in cnt)
            dxy, didp = m["depth_xy"].numpy(), m["depth_idp"].numpy()
            for b in range(count):
                assert np.array_equal(mo.bits(dxy[b, :cnt[b]]), mo.bits(xy[b, :cnt[b]])) and np.array_equal(mo.bits(didp[b, :cnt[b]]), mo.bits(idp[b, :cnt[b]]))
                assert ra[b]["n"] == rb[b]["n"] > 0 and ra[b]["tree_on_host"] == rb[b]["tree_on_host"]
            pts_dev, pts_host, cn = capi.DeviceArray((n * 8, 3), np.float64), np.zeros((n * 8, 3)), C.c_int32()
            calls = dict(reference_leg=ref_leg, new_leg=new_leg, reference_map_only=ref_map, new_map_only=new_map)
            for single in (True, False):
                tag = "single" if single else "fan8"
                calls[f"cloud_{tag}_to_host"] = lambda s=single: capi._check(LM.eds_map_window_cloud(w._h, F, c["mask"], capi.vp(T), int(s), capi.vp(pts_host), 0,
                                                                                                       C.cast(C.byref(cn), C.c_void_p), None))
                calls[f"cloud_{tag}_to_device"] = lambda s=single: capi._check(LM.eds_map_window_cloud(w._h, F, c["mask"], capi.vp(T), int(s), C.c_void_p(pts_dev.ptr),
                                                                                                         1, C.cast(C.byref(cn), C.c_void_p), None))
            for call in calls.values():
                for _ in range(a.warmup):
                    call()
            times = {k: [] for k in calls}
            for _ in range(a.reps):                               # the calls alternate
                for k, call in calls.items():
                    times[k].append(clock(call))
            rec = dict(points_per_frame=per_frame, points=n, count=count, kept=cnt.tolist(), tree_on_host=[bool(r["tree_on_host"]) for r in rb])
            rec.update({k: stats(v) for k, v in times.items()})
            rec["ratio_new_over_reference"] = rec["new_leg"]["median"] / rec["reference_leg"]["median"]
            rec["ratio_map_only_new_over_reference"] = rec["new_map_only"]["median"] / rec["reference_map_only"]["median"]
            out["cases"].append(rec)
            print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in rec.items()}))
            for t in trk:
                t.close()
            w.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
