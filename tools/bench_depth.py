"""The inverse-depth filter's update (include/eds_hip_depth.h eds_depth_update) at one alignment and at a batch of them: time per call
(host clock around calls that end in a stream synchronise, median of --reps) for the device-only source (EDS_DEPTH_REPROJECT) and for
host tracks (EDS_DEPTH_TRACKS: + the upload), with the algorithmic bytes of the kernel against the 8 TB/s HBM peak.  The kernel's own
time comes from a rocprofv3 --kernel-trace --stats run of this script (tools/README.md).
    python tools/bench_depth.py [--batches 1,4096] [--points 2000] [--reps 20] [--json out.json]"""
import argparse, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

capi = importlib.import_module("slam-eds_amd.capi")
synth = importlib.import_module("slam-eds_amd.synth")

# bytes the update kernel must move per point: seeds in and out (4 x 8 x 2), the keyframe pixel (cell 4 + two fp32 fractions),
# the plane write (4) — plus the host tracks (16, TRACKS) or the re-projection's x, y, rho planes (12, REPROJECT)
BYTES_COMMON = 64 + 12 + 4
BYTES = {"reproject": BYTES_COMMON + 12, "tracks": BYTES_COMMON + 16}
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4096")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, W, N = 120, 160, a.points
    base = [synth.make_alignment(900 + k, H=H, W=W, N=N) for k in range(8)]
    rng = np.random.default_rng(0)
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        h = capi.Handle(capi.default_config(exec=capi.EXEC_DEVICE), B, N, H, W)
        for b in range(B):
            h.set_alignment(b, base[b % 8])
        h.depth_init(0, B, capi.DEPTH_INIT_PLANE, min_depth=0.5, max_depth=6.0)
        P = rng.uniform(-0.1, 0.1, size=(B, 3))
        Q = np.array([synth.quat_from_axis_angle(rng.normal(size=3), 0.01) for _ in range(B)])
        h.set_states(0, P, Q, np.stack([base[b % 8].v0 for b in range(B)]))
        tracks = rng.normal(scale=2.0, size=(B, N, 2))
        for name, call in (("reproject", lambda: h.depth_update(0, B, capi.DEPTH_REPROJECT)),
                           ("tracks", lambda: h.depth_update(0, B, capi.DEPTH_TRACKS, xy=tracks))):
            call(); call()
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
            ms = 1e3 * float(np.median(ts))
            nbytes = BYTES[name] * B * N
            row = dict(source=name, alignments=B, points=N, call_ms=ms, algorithmic_bytes=nbytes,
                       call_GBps=nbytes / (ms * 1e-3) / 1e9, bytes_floor_us=nbytes / HBM_PEAK * 1e6)
            rows.append(row)
            print(json.dumps(row), flush=True)
        h.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
