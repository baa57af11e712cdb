"""Times the history calls of include/eds_hip_winflag.h on the device at the DSO-sized window of tools/winedit_measure.py — 2 000 points
per frame, 7 frames, every point observed in the 6 other frames — beside the route each replaces through the entry points that existed
before: for the flags eds_win_get_residuals (the states and active marks alone: the other pointers NULL) + eds_win_get_points + the decision on the host (csrc/eds_winflag.hpp under g++, what a C++
caller would run; it cannot re-linearize the chosen points, which the device call does), and for acting on them
eds_wsv_fix_linearization + eds_wsv_marginalize_points + eds_wed_remove_points with host arrays; for the fixLinearization pass eds_win_apply + eds_win_get_residuals (states and active marks) + the history's update on the host (csrc/eds_winflag.hpp under g++, what a C++ caller would run); for the new keyframe's residuals
the read-back of every row, the merge on the host and eds_win_set_residuals.  Every timed call ends with its own wait for the stream, so
a host clock around it is the call's time; the window is set up again (untimed) before every repetition.  Warm-up repetitions first;
medians.

    python tools/winflag_measure.py [--reps 30] [--out profiles/winflag_timing.json]
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

import window_cases as wc            # noqa: E402
import winflag_cases as wfc          # noqa: E402
import winflag_harness as wfh        # noqa: E402
import winsolve_cases as wsc         # noqa: E402
import winsolve_harness as wsh       # noqa: E402

window = importlib.import_module("slam-eds_amd.window")
winsolve = importlib.import_module("slam-eds_amd.winsolve")
winedit = importlib.import_module("slam-eds_amd.winedit")
winflag = importlib.import_module("slam-eds_amd.winflag")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points-per-frame", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winflag_timing.json"))
    a = ap.parse_args()
    F = a.frames
    c = wc.make(11, F, [a.points_per_frame] * F, shift=1)
    s = wsc.extend("dso", c, 111, rounds=wsc.ROUNDS["f3_513"])
    n, m = len(c.host), len(c.point)
    hist = wfc.history_for(c.host, c.point, c.target, F, 9)
    newest = F - 1
    towards = (c.target == newest).astype(np.int32)             # taken out before the insert is timed: the insert puts them back
    w = wsh.wh.open_case(c, window.Window, max_points=n, max_residuals=m + n)      # room for a residual per point
    sv = winsolve.WindowSolver(w)
    ed = winedit.WindowEdit(w, sv)
    fl = winflag.WindowFlags(w)
    wfh.load_harness()

    def states():
        """eds_win_get_residuals for the states and the active marks alone: 2 m words"""
        state, active = np.zeros(w.m, np.int32), np.zeros(w.m, np.int32)
        out = window.ResidualOut(state=state.ctypes.data, is_active=active.ctypes.data)
        window.capi._check(window._lib().eds_win_get_residuals(w._h, C.byref(out)))
        return state, active

    def setup():
        w.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
        w.set_residuals(c.point, c.target, c.state, c.energy)
        fl.set_history(**hist)
        w.linearize(F, c.precalc, c.th)

    def state_set():
        w.apply(True)
        sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
        ed.remove_residuals(towards)

    def host_pass():
        w.apply(True)
        state, active = states()
        return wfh.apply_fixed(hist, c.host, c.uv, c.ids, c.point, c.target, state, active, c.precalc, F, 0)

    def host_insert():
        res, st, rows = w.residuals(), sv.get(system=False), ed.rows()
        point, target, new_map, _ = wfh.insert_frame_residuals(hist_after, c.host, rows["point"], rows["target"], newest)
        old = new_map >= 0
        state, energy = np.zeros(len(point), np.int32), np.zeros(len(point), np.float32)
        state[old], energy[old] = res["state"], res["energy"]
        carried = {k: v for k, v in res.items()}                # every row a caller would carry over, J and the linearized rows included
        carried.update({k: st[k] for k in ("is_linearized", "res_toZeroF", "resApprox")})
        w.set_residuals(point, target, state, energy)
        return len(carried)

    hist_after = wfh.remove_residuals(hist, c.point, c.target, towards == 0)
    # the flags: about 10 % of the points leave (their latest residual went out of bounds), all of them inliers; the Hessians' median
    # as the threshold, so that half of them are marginalised and half dropped
    rng = np.random.default_rng(5)
    leaving = dict(hist, num_good=np.full(n, 10, np.int32), last_state=np.where(rng.random((n, 1)) < 0.1, 1, 0).astype(np.int32).repeat(2, axis=1))
    memo = {}

    def flags_ready():
        w.apply(True)
        sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
        w.point_hessians(s.priorF, s.deltaF)
        fl.set_history(**leaving)
        if "th" not in memo:
            memo["th"] = float(np.median(w.points()["idepth_hessian"]))

    def flagged():
        flags_ready()
        memo["totals"] = fl.flag_points(F, 0, c.precalc, c.th, min_idepth_h_marg=memo["th"])[0]
        memo["fates"] = fl.fates()

    def host_flags():
        state, pts = states()[0], w.points()
        return wfh.flag_points(leaving, c.host, c.ids, c.point, c.target, state, pts["idepth_hessian"], 0, prm=dict(min_idepth_h_marg=memo["th"]))

    def device_leave():
        return fl.marginalize_flagged(s.HM, s.bM), fl.remove_flagged()

    def host_leave():
        fates = memo["fates"]
        sv.fix_linearization(((fates == 1)[c.point] & (states()[1] != 0)).astype(np.int32))
        return sv.marginalize_points((fates == 1).astype(np.int32), s.HM, s.bM), ed.remove_points((fates != 0).astype(np.int32))

    timed = {
        "apply_fixed": (lambda: None, lambda: fl.apply_fixed(F, c.precalc, 0)),
        "apply_then_read_back_then_host_history": (lambda: None, host_pass),
        "insert_frame_residuals": (state_set, lambda: fl.insert_frame_residuals(newest)),
        "read_back_then_set_residuals": (state_set, host_insert),
        "flag_points_10pct": (flags_ready, lambda: fl.flag_points(F, 0, c.precalc, c.th, min_idepth_h_marg=memo["th"])),
        "get_residuals_get_points_then_host_decision": (flags_ready, host_flags),
        "marginalize_flagged_then_remove_flagged": (flagged, device_leave),
        "fix_marginalize_remove_with_host_flags": (flagged, host_leave),
    }
    out = dict(points=n, residuals=m, frames=F, image=[c.H, c.W], reps=a.reps, warmup=a.warmup, removed_before_the_insert=int(towards.sum()), unit="ms",
               median={}, min={}, max={}, counts={})
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
    print("fates at the flags' timing (kept, marginalised, dropped):", memo["totals"].tolist(), flush=True)
    w.close()


if __name__ == "__main__":
    main()
