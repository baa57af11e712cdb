"""Case files of oracle/_ref/ref_driver (oracle/ref/ref_driver.cpp) — test infrastructure.

write_case() lays an alignment out as the driver reads it, run() calls the driver and reads its answer back.  The driver exists only
where oracle/ref/Makefile's probe found Ceres <= 2.1 + Eigen + OpenCV + yaml-cpp + Rock base-types; available() says whether."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(os.path.dirname(HERE), "_ref", "ref_driver")
KDTREE = os.path.join(os.path.dirname(HERE), "_ref", "kdtree_nn")
NANOFLANN = os.path.join(os.path.dirname(HERE), "_ref", "nanoflann_nn")


def available() -> bool:
    return os.path.isfile(DRIVER) and os.access(DRIVER, os.X_OK)


def kdtree_available() -> bool:
    """oracle/_ref/kdtree_nn: the reference's KDTree.hpp, unmodified, with the reference's flags (built wherever the tree exists)."""
    return os.path.isfile(KDTREE) and os.access(KDTREE, os.X_OK)


def kdtree_nn(depth_xy, queries):
    """KDTree<Point2d>(depth_xy).nnSearch(query, &minDist) for every query (KeyFrame.cpp:1151-1158): (int64 index, float64 minDist)."""
    d = np.ascontiguousarray(depth_xy, dtype=np.float64).reshape(-1, 2)
    q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    with tempfile.TemporaryDirectory() as t:
        cin, cout = os.path.join(t, "case.bin"), os.path.join(t, "out.bin")
        with open(cin, "wb") as f:
            np.array([len(d)], dtype=np.int32).tofile(f); d.tofile(f)
            np.array([len(q)], dtype=np.int32).tofile(f); q.tofile(f)
        subprocess.run([KDTREE, cin, cout], check=True, stdout=subprocess.DEVNULL)
        raw = open(cout, "rb").read()
    n = len(q)
    return np.frombuffer(raw[:4 * n], dtype=np.int32).astype(np.int64), np.frombuffer(raw[4 * n:], dtype=np.float64).copy()


def nanoflann_available() -> bool:
    """oracle/_ref/nanoflann_nn: the reference's nanoflann.h, unmodified, with the reference's flags (built wherever the tree exists)."""
    return os.path.isfile(NANOFLANN) and os.access(NANOFLANN, os.X_OK)


def nanoflann_nn(uv, uv_up=None):
    """CoarseInitializer::makeNN's two searches (CoarseInitializer.cpp:888-946) for every point of uv (n x 2 fp32): the ten neighbours
    in uv and the nearest point of uv_up (None or empty: no level above) to 0.5f pt - 0.25f.  Returns dict(nb int32 n x 10, dist
    float32 n x 10 (squared, 0 where nb is -1), parent int32 n (-1 without a level above), parent_dist float32 n)."""
    p = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    u = np.zeros((0, 2), np.float32) if uv_up is None else np.ascontiguousarray(uv_up, dtype=np.float32).reshape(-1, 2)
    with tempfile.TemporaryDirectory() as t:
        cin, cout = os.path.join(t, "case.bin"), os.path.join(t, "out.bin")
        with open(cin, "wb") as f:
            np.array([len(p)], dtype=np.int32).tofile(f); p.tofile(f)
            np.array([len(u)], dtype=np.int32).tofile(f); u.tofile(f)
        subprocess.run([NANOFLANN, cin, cout], check=True, stdout=subprocess.DEVNULL)
        raw = open(cout, "rb").read()
    n = len(p)
    assert len(raw) == 4 * (22 * n), (len(raw), n)
    return dict(nb=np.frombuffer(raw[:40 * n], dtype=np.int32).reshape(n, 10).copy(),
                dist=np.frombuffer(raw[40 * n:80 * n], dtype=np.float32).reshape(n, 10).copy(),
                parent=np.frombuffer(raw[80 * n:84 * n], dtype=np.int32).copy(),
                parent_dist=np.frombuffer(raw[84 * n:], dtype=np.float32).copy())


def build() -> str:
    """Runs the recipe; returns its last line ('built ...', or 'parity unpinned: ...' where the probe fails — not an error)."""
    r = subprocess.run(["make", "-s", "-C", HERE], capture_output=True, text=True)
    lines = [l for l in (r.stdout + r.stderr).splitlines() if l.strip() and not l.startswith("make")]
    return lines[-1] if lines else ""


def write_case(path, al, p, q, v, num_threads=1, loss=0, loss_param=1.0, max_num_iterations=10, function_tolerance=1e-6):
    with open(path, "wb") as f:
        np.array([al.N, al.H, al.W, num_threads, loss, max_num_iterations], dtype=np.int32).tofile(f)
        np.array([al.fx, al.fy, al.cx, al.cy, loss_param, function_tolerance], dtype=np.float64).tofile(f)
        for a in (al.norm_coord, al.grad, al.idp, al.weights, al.frame, p, q, v):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run(al, p, q, v, **kw) -> dict:
    with tempfile.TemporaryDirectory() as d:
        cin, cout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        write_case(cin, al, p, q, v, **kw)
        subprocess.run([DRIVER, cin, cout], check=True, stdout=subprocess.DEVNULL)
        o = np.fromfile(cout, dtype=np.float64)
    return dict(p=o[0:3], q=o[3:7], v=o[7:13], usable=bool(o[13]), num_successful_steps=int(o[14]), num_unsuccessful_steps=int(o[15]),
                termination_type=int(o[16]), initial_cost=o[17], final_cost=o[18], residuals=o[19:19 + al.N])
