"""Cost of the keyframe switch for 1, 64 and 1 024 alignments x 2 000 points at VGA (include/eds_hip_kfswitch.h): the in-place batched
switch — eds_kfs_build_keyframes with EDS_KFS_DEPTH_SLOTS: projection, k-d tree, KeyFrame::create, all queued on the device, one wait
per chunk — against the route there was before, alternating in the same process: per slot eds_kfp_project_depth_map to the host, then
eds_trk_build_keyframe from the host (std::nth_element tree, two waits).  Both start from the same uploaded keyframes (uploaded again
before every repetition, not timed), take the same host images and build the same keyframes (checked once per batch size).  Host clocks
around the calls after a warm-up, medians.  It also prints eds_kfs_build_tree alone on the projected maps, and how many slots took the
host tree.

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_kfswitch.py --quick` (never together with counters).

    python tools/bench_kfswitch.py [--quick] [--reps 5]
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
capi = importlib.import_module("slam-eds_amd.capi")
synth = importlib.import_module("slam-eds_amd.synth")

DISTINCT = 8                                # distinct keyframes and images; the other slots repeat them


def _image(seed, H, W):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((H, W))
    for _ in range(3):
        img = (img + np.roll(img, 1, 0) + np.roll(img, 1, 1) + np.roll(img, -1, 0) + np.roll(img, -1, 1)) / 5.0
    return np.round(255.0 * (img - img.min()) / (img.max() - img.min())).astype(np.uint8)


def _median(fn, reps, before):
    ts = []
    for _ in range(reps):
        before()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="1 and 64 alignments, 2 repetitions")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    H, W, N = 480, 640, 2000
    sel = dict(method=capi.KF_MAX, num_points=N)
    for B in ((1, 64) if a.quick else (1, 64, 1024)):
        als = [synth.make_alignment(2000 + b, H=H, W=W, N=N) for b in range(min(B, DISTINCT))]
        imgs = [_image(70 + b, H, W) for b in range(min(B, DISTINCT))]
        h = capi.Handle(capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4), B, 2048, H, W)
        images = [imgs[b % len(imgs)] for b in range(B)]
        K = np.array([[als[b % len(als)].fx, als[b % len(als)].fy, als[b % len(als)].cx, als[b % len(als)].cy] for b in range(B)])

        def upload():
            for b in range(B):
                al = als[b % len(als)]
                h.set_keyframe(b, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)
                h.set_state(b, al.p_true, al.q_true, al.v0)

        def batched():
            return h.build_keyframes(images, None, depth="slots", vectors=False, **sel)

        def per_slot():
            out = []
            for b in range(B):
                m = h.project_depth_map(b, 1)[0]
                out.append(h.build_keyframe(b, images[b], K[b], depth_xy=m["xy"], depth_idp=m["idp"], **sel))
            return out

        upload()
        new = h.build_keyframes(images, None, depth="slots", **sel)      # warm-up of both routes, and that they build the same keyframes
        upload()
        old = per_slot()
        same = all(np.array_equal(x["idp"], y["idp"]) and np.array_equal(x["weights"], y["weights"]) and np.array_equal(x["coord"], y["coord"])
                   for x, y in zip(new, old))
        upload()
        maps = [h.project_depth_map(b, 1)[0]["xy"] for b in range(min(B, 64))]
        reps = min(a.reps, 2) if a.quick else (a.reps if B < 1024 else min(a.reps, 3))
        t_new = t_old = None
        ts_new, ts_old = [], []
        for _ in range(reps):                                            # alternating
            ts_new.append(_median(batched, 1, upload))
            ts_old.append(_median(per_slot, 1, upload))
        t_new, t_old = float(np.median(ts_new)), float(np.median(ts_old))
        h.build_tree(maps)
        t0 = time.perf_counter()
        for _ in range(reps):
            h.build_tree(maps)
        t_tree = (time.perf_counter() - t0) / reps
        print(json.dumps(dict(alignments=B, points=N, H=H, W=W, reps=reps, same_keyframes=bool(same),
                              points_kept_slot0=int(new[0]["n"]), map_points_slot0=int(len(maps[0])),
                              slots_on_host_tree=int(sum(o["tree_on_host"] for o in new)),
                              batched_switch_ms=round(t_new * 1e3, 3), per_slot_host_route_ms=round(t_old * 1e3, 3),
                              host_route_over_batched=round(t_old / t_new, 2),
                              build_tree_maps=len(maps), build_tree_call_ms=round(t_tree * 1e3, 3),
                              cpu_threads=os.environ.get("OMP_NUM_THREADS", "default"))), flush=True)
        h.close()


if __name__ == "__main__":
    main()
