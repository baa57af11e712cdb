"""Times the window's table edits (include/eds_hip_winedit.h) on the device at a DSO-sized window — 2 000 points per frame, 7 frames,
every point observed in the 6 other frames — beside the round trip each replaces through the interface that existed before:
eds_win_get_residuals + eds_win_get_points + eds_wsv_get, a numpy gather by the surviving indices, eds_win_set_points +
eds_win_set_residuals.  Every timed call ends with its own wait for the stream, so a host clock around it is the call's time; the
window is set up again (untimed) before every repetition, because an edit consumes its input.  Warm-up repetitions first; medians.

    python tools/winedit_measure.py [--reps 30] [--out profiles/winedit_timing.json]
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

import window_cases as wc            # noqa: E402
import winedit_cases as wec          # noqa: E402
import winsolve_cases as wsc         # noqa: E402
import winsolve_harness as wsh       # noqa: E402

window = importlib.import_module("slam-eds_amd.window")
winsolve = importlib.import_module("slam-eds_amd.winsolve")
winedit = importlib.import_module("slam-eds_amd.winedit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points-per-frame", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winedit_timing.json"))
    a = ap.parse_args()
    F = a.frames
    c = wc.make(11, F, [a.points_per_frame] * F, shift=1)
    s = wsc.extend("dso", c, 111, rounds=wsc.ROUNDS["f3_513"])
    n, m = len(c.host), len(c.point)
    rng = np.random.default_rng(5)
    flag = (rng.random(n) < 0.1).astype(np.int32)
    frame = 2
    hosted = (c.host == frame).astype(np.int32)
    r = wec.reduce_case(s, frame)
    w = wsh.wh.open_case(c, window.Window, max_points=n, max_residuals=m)
    sv = winsolve.WindowSolver(w)
    ed = winedit.WindowEdit(w, sv)

    def setup():
        if not setup.frames:                                    # a frame that left took its image plane with it
            w.set_frames(0, c.images)
            setup.frames = True
        w.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
        w.set_residuals(c.point, c.target, c.state, c.energy)
        wsh.lin_apply(w, s)
        sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)

    def round_trip():
        res, pts, st = w.residuals(), w.points(), sv.get(system=False)
        keep_p = flag == 0
        keep_r = keep_p[c.point]
        new_index = np.cumsum(keep_p) - 1
        gathered = {k: v[keep_r] for k, v in res.items()}       # every row a caller would carry over
        gathered.update({k: v[keep_p] for k, v in pts.items()})
        gathered.update({k: st[k][keep_r] for k in ("is_linearized", "res_toZeroF", "resApprox")})
        gathered.update({k: st[k][keep_p] for k in ("lf", "step", "idepth_scaled", "priorF")})
        w.set_points(c.host[keep_p], c.uv[keep_p], c.color[keep_p], c.weights[keep_p], gathered["idepth_scaled"], c.idz[keep_p])
        w.set_residuals(new_index[c.point[keep_r]].astype(np.int32), c.target[keep_r], gathered["state"], gathered["energy"])
        return len(gathered)

    setup.frames = True                                         # open_case set them

    def leave():
        ed.remove_points(hosted)
        setup.frames = False

    timed = {
        "remove_points_10pct": (lambda: None, lambda: ed.remove_points(flag)),
        "remove_residuals_null": (lambda: None, lambda: ed.remove_residuals(None)),
        "marginalize_frame": (leave, lambda: ed.marginalize_frame(frame, s.prior[frame], s.delta_prior[frame], s.HM, s.bM)),
        "set_state_from_device": (lambda: None, lambda: ed.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta)),
        "round_trip_remove_points_10pct": (lambda: None, round_trip),
    }
    out = dict(points=n, residuals=m, frames=F, image=[c.H, c.W], reps=a.reps, warmup=a.warmup, flagged_points=int(flag.sum()),
               words_per_residual_row=1 + 1 + 4 + 4 + 3 + 16 + 74 + 74 + 8 + 1 + 8 + 8, unit="ms", median={}, min={}, max={}, counts={})
    for name, (before, call) in timed.items():
        times = []
        for k in range(a.warmup + a.reps):
            setup()
            before()
            t0 = time.perf_counter()
            got = call()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                times.append(dt)
        out["median"][name] = float(np.median(times))
        out["min"][name], out["max"][name] = float(np.min(times)), float(np.max(times))
        out["counts"][name] = [int(w.n), int(w.m)]
        print(f"{name}: median {out['median'][name]:.3f} ms (min {out['min'][name]:.3f}, max {out['max'][name]:.3f}) -> n, m = {w.n}, {w.m}", flush=True)
        del got
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    w.close()


if __name__ == "__main__":
    main()
