"""Cost of the keyframe point-set calls on the device (include/eds_hip_kfpoints.h): eds_kfp_refine_points with erase = 0 and erase = 1
and eds_kfp_project_depth_map for 1, 64 and 4 096 alignments x 2 000 points at VGA, r = 11.  Each is a host clock around the
synchronising call after a warm-up; the erasing call gets its keyframes uploaded again before every repetition (not timed).

Beside it, alternating in the same process, the only route the library offered before: eds_trk_get_event_frame, the numpy oracle's
window loop on the host, eds_trk_set_keyframe with the kept points, eds_depth_set with their seeds.  It is timed on at most
--baseline-alignments alignments and scaled to the batch (labelled as such).

Per case it also prints the algorithmic work of k_kfp_range from the shapes: taps = alignments x points x (2r+1)^2, bytes = 4 per tap
(what the window reads; the frame they come from is H x W x 4 bytes per distinct frame), and the achieved tap rate of the call.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_kfpoints.py --quick`.

    python tools/bench_kfpoints.py [--quick] [--reps 5] [--baseline-alignments 4]
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

VEL = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
DISTINCT = 8                                # distinct keyframes and frames; the other slots repeat them and share the frames


def _upload_keyframes(h, als, B):
    for b in range(B):
        al = als[b % len(als)]
        h.set_keyframe(b, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)


def _handle(B, N, H, W):
    als = [synth.make_alignment(1000 + b, H=H, W=W, N=N) for b in range(min(B, DISTINCT))]
    h = capi.Handle(capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4), B, N, H, W)
    _upload_keyframes(h, als, B)
    for b in range(B):
        al = als[b % len(als)]
        if b < len(als):
            h.set_event_frame(b, al.frame)
        else:
            h.share_event_frame(b, b % len(als))
        h.set_state(b, al.p0, al.q0, VEL)
    return h, als


def _median(fn, reps, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _baseline(h, als, nb, r, diff):
    """the host route for slots 0 .. nb - 1: frame back, numpy window loop, keyframe and seeds up again"""
    import np_kfpoints_oracle as kp
    for b in range(nb):
        al = als[b % len(als)]
        frame = h.get_event_frame(b)
        seeds, _ = h.depth_get(b)
        keep = kp.refine(frame, kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy), diff, r)[1]
        if keep.any():
            h.set_keyframe(b, al.norm_coord[keep], al.grad[keep], al.idp[keep], al.weights[keep], al.fx, al.fy, al.cx, al.cy)
            h.depth_init(b, 1, capi.DEPTH_INIT_PLANE)
            h.depth_set(b, seeds[keep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="1 and 64 alignments, no host baseline")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-alignments", type=int, default=4)
    a = ap.parse_args()
    H, W, N, r = 480, 640, 2000, 11
    import np_kfpoints_oracle as kp
    for B in ((1, 64) if a.quick else (1, 64, 4096)):
        h, als = _handle(B, N, H, W)
        al = als[0]
        rng0 = kp.window_range(h.get_event_frame(0), kp.truncated(kp.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)), r)
        diff = float(np.median(rng0))                       # about half of the points go
        reps = a.reps if B < 4096 else min(a.reps, 3)

        def reseed():
            _upload_keyframes(h, als, B)
            h.depth_init(0, B, capi.DEPTH_INIT_PLANE)

        reseed()
        h.refine_points(0, B, diff, r, erase=False)          # warm-up (allocations, code objects)
        h.project_depth_map(0, B)
        # the C calls themselves, into buffers that exist already (the Handle methods allocate their outputs per call)
        L, ip, dp = capi.lib(), capi.C.POINTER(capi.C.c_int32), capi.C.POINTER(capi.C.c_double)
        n = np.zeros(B, dtype=np.int32)
        rng = np.zeros((B, N))
        xy, idp, src = np.ones((B, N, 2)), np.ones((B, N)), np.ones((B, N), dtype=np.int32)
        refine = lambda erase, out: capi._check(L.eds_kfp_refine_points(h._h, 0, B, diff, r, 4, 255, erase, N, out, None, n.ctypes.data_as(ip)))
        refine(0, rng.ctypes.data_as(dp))
        t_rng = _median(lambda: refine(0, None), reps)
        t_out = _median(lambda: refine(0, rng.ctypes.data_as(dp)), reps)
        t_erase = _median(lambda: refine(1, None), reps, before=reseed)
        kept = int(n[0])
        reseed()
        t_proj = _median(lambda: capi._check(L.eds_kfp_project_depth_map(h._h, 0, B, None, None, 0, 0, N, xy.ctypes.data_as(dp), idp.ctypes.data_as(dp),
                                                                         src.ctypes.data_as(ip), n.ctypes.data_as(ip))), reps)
        taps = float(B) * N * (2 * r + 1) ** 2
        rec = dict(alignments=B, points=N, H=H, W=W, r=r, event_diff=diff, kept_of_slot0=kept, reps=reps,
                   refine_erase0_no_outputs_ms=round(t_rng * 1e3, 3), refine_erase0_with_range_ms=round(t_out * 1e3, 3),
                   refine_erase1_ms=round(t_erase * 1e3, 3), project_depth_map_ms=round(t_proj * 1e3, 3),
                   taps=taps, tap_bytes=4 * taps, frame_bytes=4.0 * H * W * min(B, DISTINCT),
                   taps_per_s_of_the_call=taps / t_rng)
        if not a.quick:
            nb = min(B, a.baseline_alignments)
            reseed()
            t_base = _median(lambda: _baseline(h, als, nb, r, diff), min(reps, 3), before=reseed)
            rec.update(host_route_alignments_timed=nb, host_route_ms_scaled_to_batch=round(t_base * 1e3 * B / nb, 1),
                       host_route_over_refine_erase1=round(t_base * B / nb / t_erase, 1),
                       cpu_threads=os.environ.get("OMP_NUM_THREADS", "default"))
        print(json.dumps(rec), flush=True)
        h.close()


if __name__ == "__main__":
    main()
