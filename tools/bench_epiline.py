"""Cost of the epiline tracker on the device (include/eds_hip_epiline.h): eds_epi_track_points for 1, 8 and 64 alignments x 2 000
points at VGA, r = 3, 7, 11, uniform and edge layouts.  Each alignment's event frame holds its model image shifted by a few pixels
over the synthetic event frame, so the matches are real ones.

Reports per case the call time (erase = 0, so every repeat runs the same work), the dense-equivalent multiply-adds per second
(H W N (2r+1)^2 per alignment: what a dense implicit GEMM would do) and that rate as a fraction of the fp32 matrix peak (157.3 TFLOP/s,
2 flops per multiply-add).  --cpu adds the numpy oracle's time per alignment, measured on a sample of points and scaled to 2 000
(labelled as such).  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_epiline.py --quick`.

    python tools/bench_epiline.py [--quick] [--cpu] [--reps 5]
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

PEAK_FP32_MATRIX = 157.3e12
VEL = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])


def _handle(B, N, H, W, layout):
    als = [synth.make_alignment(1000 + (b % 8), H=H, W=W, N=N, layout=layout) for b in range(min(B, 8))]
    cfg = capi.default_config(solver=capi.SOLVER_LM6, exec=capi.EXEC_DEVICE, max_num_iterations=4)
    h = capi.Handle(cfg, B, N, H, W)
    for b in range(B):
        al = als[b % len(als)]
        h.set_alignment(b, al)
        h.set_state(b, al.p0, al.q0, VEL)
        if b < len(als):
            m = h.epi_get_model(b)
            f = np.roll(m, (2, -3), axis=(0, 1)) + 0.2 * np.abs(m).max() * al.frame / np.abs(al.frame).max()
            h.set_event_frame(b, f)
            h.set_state(b, al.p0, al.q0, VEL)
        else:
            h.share_event_frame(b, b % len(als))
    return h, als


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="1 and 8 alignments, r = 7, uniform only")
    ap.add_argument("--cpu", action="store_true", help="also time the numpy oracle per alignment (sampled, scaled to N)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    H, W, N = 480, 640, 2000
    batches = (1, 8) if a.quick else (1, 8, 64)
    radii = (7,) if a.quick else (3, 7, 11)
    layouts = ("uniform",) if a.quick else ("uniform", "edges")
    for layout in layouts:
        for B in batches:
            h, als = _handle(B, N, H, W, layout)
            for r in radii:
                h.epi_track_points(0, B, r, erase=False)                # warm-up (allocations, code objects)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    h.epi_track_points(0, B, r, erase=False)
                    ts.append(time.perf_counter() - t0)
                t = float(np.median(ts))
                macs = float(B) * H * W * N * (2 * r + 1) ** 2
                rec = dict(layout=layout, alignments=B, points=N, H=H, W=W, r=r, call_ms=round(t * 1e3, 3),
                           ms_per_alignment=round(t * 1e3 / B, 3), dense_equiv_macs_per_s=macs / t,
                           frac_fp32_matrix_peak=round(2 * macs / t / PEAK_FP32_MATRIX, 4))
                if a.cpu and B == 1:
                    import np_epiline_oracle as eo
                    al = als[0]
                    kp = eo.slot_pixels(al.norm_coord, al.fx, al.fy, al.cx, al.cy)
                    g = np.asarray(al.grad, np.float64).astype(np.float32).astype(np.float64)
                    idp = np.asarray(al.idp, np.float64).astype(np.float32).astype(np.float64)
                    n_s = 16
                    t0 = time.perf_counter()
                    eo.track_points_along_epiline(kp, g, idp, VEL, (al.fx, al.fy, al.cx, al.cy), h.get_event_frame(0), r,
                                                  sample=np.arange(n_s))
                    tc = time.perf_counter() - t0
                    rec["cpu_numpy_oracle_ms_per_alignment_scaled"] = round(tc * 1e3 * N / n_s, 1)
                    rec["cpu_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
                print(json.dumps(rec), flush=True)
            h.close()


if __name__ == "__main__":
    main()
