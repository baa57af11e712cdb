"""The KLT point trackers (include/eds_hip_klt.h) at 1, 64 and 4 096 alignments x 2 000 points on VGA frames: trackPoints (r = 7) and
trackPointsPyr (L = 3), uniform and edge points.  Per case: time per call (host clock around calls that end in a stream synchronise,
median of --reps; includes getCoord and the outputs' copies), the algorithmic bytes of the KLT kernels — point data plus the DISTINCT
event-frame tiles (4 x 4 fp32, 64 B) the windows touch, counted from the returned coordinates — and the fraction of 8 TB/s those
bytes would take at the kernel times.  The kernel times themselves come from a rocprofv3 --kernel-trace --stats run of this script
(tools/README.md).
    python tools/bench_klt.py [--batches 1,64,4096] [--points 2000] [--reps 5] [--json out.json]"""
import argparse, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

capi = importlib.import_module("slam-eds_amd.capi")
synth = importlib.import_module("slam-eds_amd.synth")

HBM_PEAK = 8.0e12
# per point, what the bin and window kernels must read or write once: coordinates (16, read by both), the key (8 written, 8 read
# back, 8 sorted), the gradients of the point (8), tracks and flow (2 x 16 read-modify-write of tracks, 16 flow)
BYTES_POINT = 16 + 16 + 24 + 8 + 32 + 32


def frame_tiles(coord, r, H, W):
    """distinct 4 x 4 tiles of the event frame read by the (2r+1)^2 reflect-101 windows at the truncated coordinates"""
    c = coord[np.isfinite(coord).all(1)]
    tx, ty = np.trunc(c[:, 0]).astype(np.int64), np.trunc(c[:, 1]).astype(np.int64)
    k = np.arange(-r, r + 1)

    def refl(p, n):
        p = np.abs(p)
        return np.where(p >= n, 2 * n - 2 - p, p)

    cols = refl(tx[:, None] + k[None, :], W) >> 2
    rows = refl(ty[:, None] + k[None, :], H) >> 2
    tw = (W + 3) // 4
    ids = (rows[:, :, None] * tw + cols[:, None, :]).reshape(-1)
    return int(np.unique(ids).size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, W, N = 480, 640, a.points
    rows = []
    for layout in ("uniform", "edges"):
        base = [synth.make_alignment(700 + k, H=H, W=W, N=N, layout=layout) for k in range(8)]
        for B in [int(x) for x in a.batches.split(",")]:
            h = capi.Handle(capi.default_config(exec=capi.EXEC_DEVICE), B, N, H, W)
            for b in range(B):
                al = base[b % 8]
                h.set_keyframe(b, al.norm_coord, al.grad, al.idp, al.weights, al.fx, al.fy, al.cx, al.cy)
                if b < 8:
                    h.set_event_frame(b, al.frame)
                else:
                    h.share_event_frame(b, b % 8)
                h.set_state(b, al.p0, al.q0, al.v0)
            for name, r, call in (("track_points_r7", 7, lambda: h.klt_track_points(0, B, 7)),
                                  ("track_points_pyr_L3", 7, lambda: h.klt_track_points_pyr(0, B, 3))):
                outs = call()
                ts = []
                for _ in range(a.reps):
                    t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
                ms = 1e3 * float(np.median(ts))
                # distinct tiles per alignment (the 8 frames are shared: count the tiles of each distinct frame once per alignment
                # that reads it, as a kernel without cross-alignment reuse must)
                tiles = sum(frame_tiles(outs[b]["coord"], r, H, W) for b in range(min(B, 8)))
                tiles = tiles * B / min(B, 8)
                nbytes = BYTES_POINT * sum(o["n"] for o in outs) + 64 * tiles
                row = dict(case=name, layout=layout, alignments=B, points=N, call_ms=ms, algorithmic_bytes=int(nbytes),
                           frame_tile_bytes=int(64 * tiles), bytes_floor_us=nbytes / HBM_PEAK * 1e6)
                rows.append(row)
                print(json.dumps(row), flush=True)
            h.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
