"""Cost of tracing immature points (include/eds_hip_immature.h) on one MI355X at 640 x 480 with 2 000 points per host frame, for 1, 7
and 64 host frames: the FIRST trace of fresh points (idepth_max = NaN: lines of about 30 steps) and the FOURTH trace along the path
(short lines).  Per row: the median host-clock time around eds_imm_trace (it returns when the results are on the host) after a
warm-up, and, alternating with it in the same process, csrc/eds_immature.hpp (edsimm::, the same code on the CPU, tests/
immature_harness.py) on one thread and on 16.  Every repetition starts from the same points (restored before the clock starts).  The
device's result is compared with the CPU's once per row, bit for bit.  taps: 8 per search step; bytes: 16 per tap (the 2 x 2 footprint).

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_immature.py --hosts 7 --no-cpu` (never with counters).

    python tools/bench_immature.py [--hosts 1 7 64] [--reps 7] [--no-cpu]
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
immature = importlib.import_module("slam-eds_amd.immature")
import immature_cases as ic          # noqa: E402
import immature_harness as ih        # noqa: E402
import np_immature_oracle as no      # noqa: E402

H, W, N, K4 = 480, 640, 2000, (535.0, 530.0, 322.5, 238.25)
DISTINCT = 8                          # distinct host frames; the other hosts repeat them
THREADS = 16


def scene(hosts):
    sc = ic.Scene(2024, H, W, K4)
    rng = sc.rng
    poses = [(ic.rot(*rng.uniform(-0.01, 0.01, 2), rng.uniform(-0.03, 0.03)), np.append(rng.uniform(-0.01, 0.01, 2), 0.0)) for _ in range(min(hosts, DISTINCT))]
    himg = [sc.render(R, p) for R, p in poses]
    uv = [np.stack([rng.integers(8, W - 8, N), rng.integers(8, H - 8, N)], axis=1).astype(np.int32) for _ in poses]
    targets, pre = [], []
    for k in range(4):
        Rt, pt = ic.rot(0.002 * k, -0.003 * k, 0.004 * k), np.array([0.03, 0.004, 0.002]) * (k + 1)
        targets.append(sc.render(Rt, pt))
        pre.append([ic.precalc32(K4, Rt.T @ R, Rt.T @ (p - pt))[:3] for R, p in poses])
    return himg, uv, targets, pre


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, nargs="+", default=[1, 7, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_immature needs a GPU: libeds_hip has no CPU fallback")
    hl = ih.load_harness()
    prm = no.params()
    prm_bytes = ih.pack_params(prm)
    pool = ThreadPoolExecutor(THREADS)
    for B in a.hosts:
        himg, uv, targets, pre = scene(B)
        D = len(himg)
        h = immature.ImmaturePoints(H, W, B, N, 4)
        h.set_host_images(0, np.stack([himg[b % D] for b in range(B)]))
        h.set_target_images(0, np.stack(targets))
        grads = [ih.gradient(hl, t) for t in targets]
        args = [tuple(np.stack([pre[k][b % D][j] for b in range(B)]) for j in range(3)) for k in range(4)]

        def gpu_prepare(upto):
            for b in range(B):
                h.create_points(b, uv[b % D])
            for k in range(upto):
                h.trace(0, [k] * B, *args[k])

        def cpu_prepare(upto):
            pts = [ih.construct(hl, himg[d], uv[d], np.ones(N, np.float32), None, None, prm) for d in range(D)]
            for k in range(upto):
                for d in range(D):
                    ih.trace_g(hl, pts[d], targets[k], grads[k], prm_bytes, *pre[k][d])
            return pts

        def cpu_trace(pts, k, threads):
            jobs = [(b, s) for b in range(B) for s in range(0, N, 125)]
            run = lambda j: ih.trace_g(hl, pts[j[0]][j[1]:j[1] + 125], targets[k], grads[k], prm_bytes, *pre[k][j[0] % D])
            if threads == 1:
                for j in jobs:
                    run(j)
            else:
                list(pool.map(run, jobs))

        for k, label in ((0, "first"), (3, "fourth")):
            base = cpu_prepare(k)
            steps = np.concatenate([ih.line_steps(hl, base[b % D], H, W, prm, pre[k][b % D][0], pre[k][b % D][1]) for b in range(B)])
            t_gpu, t_c1, t_c16 = [], [], []
            gpu_prepare(k)
            h.trace(0, [k] * B, *args[k])                                         # warm-up
            for _ in range(a.reps):                                               # alternating
                gpu_prepare(k)
                t0 = time.perf_counter()
                h.trace(0, [k] * B, *args[k])
                t_gpu.append(time.perf_counter() - t0)
                if a.no_cpu:
                    continue
                for threads, ts in ((1, t_c1), (THREADS, t_c16)):
                    pts = [base[b % D].copy() for b in range(B)]
                    t0 = time.perf_counter()
                    cpu_trace(pts, k, threads)
                    ts.append(time.perf_counter() - t0)
            same = None
            if not a.no_cpu:
                same = all(no.same_bits(h.get(b)[g], pts[b][f]).all() for b in range(min(B, DISTINCT))
                           for f, g in (("idepth_min", "idepth_min"), ("idepth_max", "idepth_max"), ("quality", "quality"),
                                        ("status", "lastTraceStatus"), ("last_uv", "lastTraceUV"), ("last_interval", "lastTracePixelInterval")))
            taps = 8 * int(steps.sum())
            g = float(np.median(t_gpu))
            row = dict(hosts=B, points_per_host=N, H=H, W=W, trace=label, reps=a.reps, searched_points=int((steps > 0).sum()),
                       median_steps=float(np.median(steps[steps > 0])) if (steps > 0).any() else 0.0, search_taps=taps,
                       search_bytes_requested=16 * taps, frame_bytes=4 * H * W, gpu_call_ms=round(g * 1e3, 4),
                       gpu_search_taps_per_s=round(taps / g, 1), device_equals_cpu=same)
            if not a.no_cpu:
                row.update(cpu_1_thread_ms=round(float(np.median(t_c1)) * 1e3, 3), cpu_16_threads_ms=round(float(np.median(t_c16)) * 1e3, 3),
                           cpu_1_over_gpu=round(float(np.median(t_c1)) / g, 1), cpu_16_over_gpu=round(float(np.median(t_c16)) / g, 1))
            print(json.dumps(row), flush=True)
        h.close()


if __name__ == "__main__":
    main()
