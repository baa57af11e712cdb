"""Cost of the rest of the window's iteration (include/eds_hip_winsolve.h) on one MI355X at the size of tools/bench_window.py: 640 x 480,
F = 7 frames, 2 000 points per host frame.  Per call (eds_wsv_fix_linearization, eds_wsv_solve, eds_wsv_l_energy, eds_wsv_m_energy,
eds_wsv_backup_idepths, eds_wsv_step_idepths, and one eds_wsv_marginalize_points at the end): the median of `reps` host-clock times after
a warm-up, alternating in the same process with edswsv:: (csrc/eds_winsolve.hpp, the same code on the CPU, tests/winsolve_harness.py) on
one thread; what both sides return is compared bit for bit in every repetition.

And the whole iteration two ways, no residual linearized (the parent route cannot take any):
  device   eds_win_linearize, eds_win_apply, eds_wsv_solve, eds_wsv_step_idepths: nothing but x comes back;
  parent   eds_win_linearize, eds_win_apply, eds_win_accumulate (four matrices come back), the priors, the assembly and a scaled solve in
           numpy, the per-point sums and JpJdF downloaded, resubstituteFPt in numpy, eds_win_set_idepths.
The two routes do not give the same bits (numpy's solve is LAPACK's); the largest difference of the steps is printed.  No gate.

Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/bench_winsolve.py --no-cpu` (never with counters).

    python tools/bench_winsolve.py [--reps 7] [--no-cpu]
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
capi = importlib.import_module("slam-eds_amd.capi")
window = importlib.import_module("slam-eds_amd.window")
winsolve = importlib.import_module("slam-eds_amd.winsolve")
import window_cases as wc            # noqa: E402
import winsolve_cases as wsc         # noqa: E402
import winsolve_harness as wsh       # noqa: E402

H, W, F, PER_HOST, K4 = 480, 640, 7, 2000, (535.0, 530.0, 322.5, 238.25)
CALLS = ("fix_linearization", "backup_idepths", "solve", "l_energy", "m_energy", "step_idepths")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def one_round(w, sv, s, fac):
    """the calls of one iteration after linearize -> apply; returns (seconds per call, what they returned)"""
    t = {}
    t["fix_linearization"], _ = timed(lambda: sv.fix_linearization(s.fix))
    t["backup_idepths"], _ = timed(sv.backup_idepths)
    t["solve"], sol = timed(lambda: sv.solve(2, 0.0, s.HM, s.bM, wsc.DEFAULT, True, s.P))
    t["l_energy"], le = timed(sv.l_energy)
    t["m_energy"], me = timed(lambda: sv.m_energy(s.HM, s.bM))
    steps = sv.steps()
    t["step_idepths"], _ = timed(lambda: sv.step_idepths(fac))
    ids = sv.get(system=False)["idepth_scaled"]
    wsh.lin_apply(w, s)
    return t, dict(x=sol["x"], lastHS=sol["lastHS"], lastbS=sol["lastbS"], l_energy=np.float64(le), m_energy=np.float64(me), steps=steps, idepth_scaled=ids)


def parent_route(w, s, c):
    """accumulate on the device, everything after it on the host, as a caller of the parent commit has to"""
    N = s.N
    acc = w.accumulate(c.F, c.adH, c.adT, s.priorF, s.deltaF, None, True)
    prior = np.concatenate([s.cPrior, s.prior.ravel()])
    d = np.concatenate([s.cDelta.astype(np.float32).astype(np.float64), s.delta.ravel()])
    bL = np.concatenate([s.cPrior * d[:4], (s.prior * s.delta_prior).ravel()])
    lam = 1e-5
    Hf = np.diag(prior) + s.HM + acc["H_A"]
    bf = bL + (s.bM + s.HM @ d) + acc["b_A"] - acc["b_sc"]
    Hf[np.diag_indices(N)] *= 1 + lam
    Hf -= acc["H_sc"] * (1.0 / (1 + lam))
    S = 1.0 / np.sqrt(np.diag(Hf) + 10.0)
    x = S * np.linalg.solve((S[:, None] * Hf) * S[None, :], S * bf)
    x = x - s.P @ x
    pts = w.points()
    JpJdF, active = np.zeros((w.m, 8), np.float32), np.zeros(w.m, np.int32)
    out = window.ResidualOut(JpJdF=JpJdF.ctypes.data, is_active=active.ctypes.data)
    capi._check(window._lib().eds_win_get_residuals(w._h, C.byref(out)))
    xF = x.astype(np.float32)
    adHF, adTF = c.adH.astype(np.float32), c.adT.astype(np.float32)
    xAd = np.zeros((c.F, c.F, 8), np.float32)
    for h in range(c.F):
        for t in range(c.F):
            xAd[h, t] = xF[4 + 8 * h:12 + 8 * h] @ adHF[h + c.F * t] + xF[4 + 8 * t:12 + 8 * t] @ adTF[h + c.F * t]
    b = pts["bdSumF"] - pts["Hcd_accAF"] @ xF[:4]
    dots = np.einsum("rk,rk->r", xAd[c.host[c.point], c.target], JpJdF) * (active != 0)
    b = b - np.bincount(c.point, weights=dots, minlength=w.n).astype(np.float32)
    step = np.where(pts["nres"] > 0, -b * pts["HdiF"], 0).astype(np.float32)
    return x, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_winsolve needs a GPU: libeds_hip has no CPU fallback")
    c = wc.make(2026, F, [PER_HOST] * F, shift=1, shape=(H, W), K=K4)
    s = wsc.extend("bench", c, 2026, rounds=[])
    n, m = s.n, s.m
    sides = {"device": wsh.open_case(s, window.Window, winsolve.WindowSolver, max_points=n, max_residuals=m)}
    if not a.no_cpu:
        sides["cpu_1_thread"] = wsh.open_case(s)
    for w, sv in sides.values():
        wsh.lin_apply(w, s)
        sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
        one_round(w, sv, s, 0.25)                               # warm-up
    times = {k: {q: [] for q in CALLS} for k in sides}
    equal = True
    for rep in range(a.reps):
        out = {}
        for k, (w, sv) in sides.items():
            t, out[k] = one_round(w, sv, s, 0.25 if rep % 2 else -0.25)
            for q in CALLS:
                times[k][q].append(t[q])
        if "cpu_1_thread" in out:
            equal = equal and all(wsh.same_bits(out["device"][f], out["cpu_1_thread"][f]) for f in out["device"])
    marg = {}
    for k, (w, sv) in sides.items():
        sv.fix_linearization(s.fix_marg)
        marg[k], res = timed(lambda: sv.marginalize_points(s.marg, s.HM, s.bM, wsc.PRIOR_FAC, wsc.WEIGHT_FAC))
        out[k] = dict(HM=res[0], bM=res[1])
    if "cpu_1_thread" in out:
        equal = equal and all(wsh.same_bits(out["device"][f], out["cpu_1_thread"][f]) for f in out["device"])
    # the whole iteration, two ways, no residual linearized
    w, sv = sides["device"]
    w.set_points(c.host, c.uv, c.color, c.weights, c.ids, c.idz)
    w.set_residuals(c.point, c.target, c.state, c.energy)
    wsh.lin_apply(w, s)
    sv.set_state(s.F, c.adH, c.adT, s.delta, s.prior, s.delta_prior, s.cPrior, s.cDelta, s.priorF, s.deltaF)
    sv.backup_idepths()
    loop_dev, loop_par, diff = [], [], 0.0
    for rep in range(a.reps + 1):
        def device_iteration():
            w.linearize(c.F, c.precalc, c.th)
            w.apply(True)
            sv.solve(2, 0.0, s.HM, s.bM, wsc.DEFAULT, True, s.P)
            sv.step_idepths(0.0)                                 # fac 0: the next repetition starts from the same point
        td, _ = timed(device_iteration)
        dev_step = sv.steps()

        def parent_iteration():
            w.linearize(c.F, c.precalc, c.th)
            w.apply(True)
            x, step = parent_route(w, s, c)
            w.set_idepths(c.ids + np.float32(0.0) * step)
            return step
        tp, par_step = timed(parent_iteration)
        if rep:
            loop_dev.append(td)
            loop_par.append(tp)
        diff = max(diff, float(np.max(np.abs(dev_step - par_step) / (np.abs(dev_step) + 1e-3))))
    med = {k: {q: float(np.median(v)) for q, v in ts.items()} for k, ts in times.items()}
    row = dict(H=H, W=W, F=F, N=s.N, points=n, residuals=m, linearized=int(s.fix.sum()), marginalised=int(s.marg.sum()), reps=a.reps)
    for k in sides:
        for q in CALLS:
            row[f"{k}_{q}_ms"] = round(med[k][q] * 1e3, 4)
        row[f"{k}_marginalize_points_ms"] = round(marg[k] * 1e3, 4)
    if not a.no_cpu:
        row["cpu_1_thread_equals_device"] = bool(equal)
    row.update(iteration_device_ms=round(float(np.median(loop_dev)) * 1e3, 4), iteration_parent_route_ms=round(float(np.median(loop_par)) * 1e3, 4),
               iteration_step_rel_diff=diff)
    print(json.dumps(row), flush=True)
    w.close()


if __name__ == "__main__":
    main()
