"""Hand-over of inputs that already live in device memory (include/eds_hip_device.h) against the host entry points, same process,
the two paths alternating: 256 VGA event frames (fp32 and fp64) through eds_dev_set_event_frames / eds_trk_set_event_frames[_f32], and
256 keyframes of 2 000 points through eds_dev_set_keyframes / eds_trk_set_keyframe.  Host clock around call + sync for both paths,
HIP events on the handle's stream for the device path, and the copy rate eds_trk_hbm_probe reports on the same box to hold the
store kernel's bytes/s against.

    python tools/bench_device_inputs.py [--reps 7] [--out profiles/device_inputs.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_device_inputs.py --device-only     # kernel times of their own
"""
import argparse, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
capi = importlib.import_module("slam-eds_amd.capi")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--device-only", action="store_true", help="only the device path (a profiler run: no host-path kernels in the trace)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

H, W, B, N = 480, 640, 256, 2000
Hp, Wp = ((H + 3) & ~3) + 8, ((W + 3) & ~3) + 8
rng = np.random.default_rng(0)
h = capi.Handle(capi.default_config(exec=capi.EXEC_DEVICE), B, N, H, W)
med = lambda v: float(np.median(v))
res = {"H": H, "W": W, "frames": B, "keyframes": B, "points": N, "reps": args.reps}


def wall(f):
    t = time.perf_counter(); f(); h.sync()
    return 1e3 * (time.perf_counter() - t)


def device(f):
    """(host time of the call itself, device time between two events on the handle's stream), ms"""
    h.timer_start(); t = time.perf_counter(); f(); call = 1e3 * (time.perf_counter() - t)
    return call, h.timer_stop()


base = rng.standard_normal((8, H, W)) * 1e-2
for dt in (np.float32, np.float64):
    fr = np.ascontiguousarray(np.stack([base[i % 8] + i for i in range(B)]), dtype=dt)
    host_list = [fr[i] for i in range(B)]
    d = capi.DeviceArray.from_numpy(fr)
    dev_call = lambda: h.set_event_frames_device(0, d)
    host_call = lambda: h.set_event_frames(0, host_list)
    wall(dev_call); args.device_only or wall(host_call)             # warm-up: staging ring, code objects
    wd, wh, ev, call = [], [], [], []
    for _ in range(args.reps):                                      # alternating
        wd.append(wall(dev_call))
        if not args.device_only:
            wh.append(wall(host_call))
        c, e = device(dev_call); call.append(c); ev.append(e)
    nbytes = B * (fr.dtype.itemsize * H * W + 4 * Hp * Wp)
    res["frames_" + np.dtype(dt).name] = {
        "device_wall_ms": med(wd), "host_wall_ms": med(wh) if wh else None, "device_call_ms": med(call), "device_event_ms": med(ev),
        "bytes_moved": nbytes, "device_GBps_by_events": nbytes / med(ev) / 1e6, "us_per_frame_by_events": 1e3 * med(ev) / B}
    h.sync(); d.free()

# keyframes: rows `N + 7` points apart, a K per slot
S = N + 7
nc, g = rng.uniform(-0.4, 0.4, (B, S, 2)), rng.standard_normal((B, S, 2))
idp, w = rng.uniform(0.2, 1.0, (B, S)), rng.uniform(0.7, 1.0, (B, S))
K = np.tile([500.0, 500.0, 319.5, 239.5], (B, 1)) + rng.uniform(-1, 1, (B, 4))
darr = [capi.DeviceArray.from_numpy(a) for a in (nc, g, idp, w)]
Ns = [N] * B
dev_call = lambda: h.set_keyframes_device(0, Ns, *darr, K)
host_call = lambda: [h.set_keyframe(b, nc[b, :N], g[b, :N], idp[b, :N], w[b, :N], *K[b]) for b in range(B)]
wall(dev_call); args.device_only or wall(host_call)
wd, wh, ev, call = [], [], [], []
for _ in range(args.reps):
    wd.append(wall(dev_call))
    if not args.device_only:
        wh.append(wall(host_call))
    c, e = device(dev_call); call.append(c); ev.append(e)
res["keyframes"] = {"device_wall_ms": med(wd), "host_wall_ms": med(wh) if wh else None, "device_call_ms": med(call),
                    "device_event_ms": med(ev), "note": "device_event_ms covers the pose upload, k_ingest_points and the Gram launch"}
if not args.device_only:
    res["hbm_probe"] = h.hbm_probe(1 << 30, 10)
h.sync()
for a in darr:
    a.free()
h.close()
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
