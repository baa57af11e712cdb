"""Times eds_und_process (include/eds_hip_undistort.h) on the device: uint8 frames, photometric_calibration 2, at 640 x 480 and
1280 x 1024, 1 and 16 frames a call, in both device forms — FUSED (one kernel) and TWO_PASS (photometric plane, then remap) — and under
the default AUTO, which chooses between them by the size of the call, with the
raw frames in host memory (the call then includes their upload) and already in device memory.  The forms alternate inside one
loop, so that whatever else the machine is doing falls on both.  For scale, what a caller does without eds_und: the host restatement
edsund:: (csrc/eds_undistort.hpp under g++ -O2, one thread) for every frame plus one eds_sel_set_image upload of the fp32 plane.

Every timed call ends with its own wait for the stream, so a host clock around it is the call's time.  Warm-up repetitions first;
medians, with the minimum and maximum beside them.  Before anything is timed the two forms and the host restatement are compared bit
for bit on the very frames that are timed.

    python tools/bench_undistort.py [--reps 2000] [--out profiles/undistort_timing.json]
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

import np_undistort_oracle as uo     # noqa: E402
import undistort_cases as uc         # noqa: E402
import undistort_harness as uh       # noqa: E402

capi = importlib.import_module("slam-eds_amd.capi")
und = importlib.import_module("slam-eds_amd.undistort")
select = importlib.import_module("slam-eds_amd.select")
FORMS = {"fused": und.FORM_FUSED, "two_pass": und.FORM_TWO_PASS, "auto": und.FORM_AUTO}


def clock(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    return dict(median=float(np.median(times)), min=float(np.min(times)), max=float(np.max(times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_timing.json"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_undistort needs a GPU: nothing here is measured without one")
    out = dict(unit="ms", raw="uint8", photometric_calibration=2, reps=a.reps, host_reps=a.host_reps, warmup=a.warmup, default_form=None, cases=[])
    pars = [0.535719308086809, 0.669566858850269, 0.493248545285398, 0.500408664348414, 0.897966326944875]
    for (w, h) in ((640, 480), (1280, 1024)):
        g = und.geometry(uo.FOV, pars, w, h, uo.CROP, w, h)
        G, vig = uc.gamma_table(256), uc.vignette(h, w)
        host = uh.HostUndistorter(g)
        host.set_photometric(G, vig)
        sel = select.Selector(h, w)
        for count in (1, 16):
            raw = uc.raw_frames(count, h, w, 40 + count)
            exposures = [0.02] * count
            u = und.Undistorter(g, slots=count)
            if out["default_form"] is None:
                out["default_form"] = [k for k, v in FORMS.items() if v == u.form][0]
                out["auto_is_two_pass_from_raw_pixels"] = 4 << 20
            u.set_photometric(G, vig)
            d_raw = capi.DeviceArray.from_numpy(raw)
            # the timed work gives the same bits in both forms, and the host restatement's
            host.process(raw, exposures)
            want = host.planes.copy()
            for form in FORMS.values():
                u.form = form
                u.process(d_raw, exposures)
                assert all(uc.same_bits(u.get_image(k), want[k]) for k in range(count)), "the device and edsund:: differ"
            t = {f"{name}_{src}": [] for name in FORMS for src in ("host_raw", "device_raw")}
            for k in range(a.warmup + a.reps):
                for name, form in FORMS.items():
                    u.form = form
                    dt_h = clock(lambda: u.process(raw, exposures))
                    dt_d = clock(lambda: u.process(d_raw, exposures))
                    if k >= a.warmup:
                        t[f"{name}_host_raw"].append(dt_h)
                        t[f"{name}_device_raw"].append(dt_d)
            th, tu = [], []
            for k in range(1 + a.host_reps):
                dt_h = clock(lambda: host.process(raw, exposures))
                planes = host.planes
                dt_u = clock(lambda: [sel.set_image(planes[i]) for i in range(1)])
                if k >= 1:
                    th.append(dt_h)
                    tu.append(dt_u)
            case = dict(w=w, h=h, count=count, **{k: stats(v) for k, v in t.items()}, host_edsund_all_frames=stats(th),
                        one_eds_sel_set_image_upload=stats(tu), host_edsund_plus_one_upload=stats(np.add(th, tu)))
            out["cases"].append(case)
            print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in case.items()}), flush=True)
            u.close()
        sel.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
