"""numpy restatement of what include/eds_hip_kfpoints.h computes: KeyFrame::pointsRefinement's window range and decision,
KeyFrame::cleanPoints, KeyFrame::erasePoint, the KeyFrame::num_points rules, and the keyframe switch getDepthMap() -> T_dst_src ->
IDepthMap::fromPoints in the header's order of operations.  Pure numpy, fed what a tracker slot holds (np_epiline_oracle.slot_pixels,
the frame as eds_trk_get_event_frame returns it)."""
import warnings

import numpy as np

from np_epiline_oracle import (BORDER_CONSTANT, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, border_index, slot_pixels,  # noqa: F401
                               take_bordered)

TRUNC_MAX = 2.0 ** 20          # a truncated pixel coordinate beyond +-2^20 is taken as +-2^20 (the header)


def truncated(kpix):
    """cv::Rect of a Point2d: the slot's pixel (cell + fp32 fraction) TRUNCATED, (tx, ty) as int64"""
    kp = np.clip(np.asarray(kpix, dtype=np.float64), -TRUNC_MAX, TRUNC_MAX)
    return np.trunc(kp[:, 0]).astype(np.int64), np.trunc(kp[:, 1]).astype(np.int64)


def window_range(frame, centres, r, border=BORDER_REFLECT_101, value=255):
    """|max - min| of the (2r+1)^2 window of `frame` (the stored fp32 values) around every integer centre (tx, ty), in fp64; min and
    max ignore NaN taps, a window without a finite tap gives NaN"""
    tx, ty = centres
    k = np.arange(2 * r + 1)
    f32 = np.asarray(frame).astype(np.float32)
    out = np.empty(len(tx))
    for s in range(0, len(tx), 256):          # N x S x S taps at a time
        w = take_bordered(f32, ty[s:s + 256, None] - r + k[None, :], tx[s:s + 256, None] - r + k[None, :], border, value).astype(np.float32)
        w = w.reshape(len(w), -1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)       # an all-NaN window
            lo, hi = np.nanmin(w, axis=1), np.nanmax(w, axis=1)
        out[s:s + 256] = np.abs(hi.astype(np.float64) - lo.astype(np.float64))
    return out


def refine(frame, kpix, event_diff, r=11, border=BORDER_REFLECT_101, value=255, centres=None):
    """pointsRefinement: (range, keep mask).  A point is erased iff range < event_diff; a NaN range is kept"""
    rng = window_range(frame, truncated(kpix) if centres is None else centres, r, border, value)
    return rng, ~(rng < float(event_diff))


def clean(weights, w_norm_thr):
    """cleanPoints: keep mask of the stored fp32 weights, widened, against the threshold"""
    w = np.asarray(weights, dtype=np.float64).astype(np.float32).astype(np.float64)
    return ~(w < float(w_norm_thr))


def erase(n, which):
    """erasePoint for a boolean mask or an index list: keep mask"""
    keep = np.ones(n, bool)
    w = np.asarray(which)
    if w.dtype == np.bool_:
        keep &= ~w
    else:
        keep[w.astype(np.int64)] = False
    return keep


class NumPoints:
    """KeyFrame::num_points and coord.size() through the calls that touch a slot's point set"""

    def __init__(self):
        self.num_points, self.current = 0, 0

    def set_keyframe(self, n):                  # eds_trk_set_keyframe, eds_dev_set_keyframes, eds_pyr_*
        self.num_points = self.current = int(n)

    def build_keyframe(self, candidates, n):    # candidatePoints assigns num_points (KeyFrame.cpp:820); cleanPoints leaves it
        self.num_points, self.current = int(candidates), int(n)

    def refine(self, kept, erased=True):        # KeyFrame.cpp:1056
        if erased:
            self.num_points = self.current = int(kept)

    def erased(self, kept):                     # cleanPoints, erasePoint, getCoord(true), the KLT, the epiline cull
        self.current = int(kept)

    def need_new_kf(self, percent_thr=0.1):     # unsigned int - size_t: wraps (KeyFrame.cpp:1556)
        return float((self.num_points - self.current) % (1 << 64)) > percent_thr * float(self.num_points)

    def need_new_kf_image(self, percent, rows, cols):
        return float(self.current) < float(cols * rows) * percent


def quat_to_R(q, dtype=np.float64):
    """R of the normalised quaternion (x, y, z, w), entry by entry as the library forms it on the host"""
    q = np.asarray(q, dtype=dtype)
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    x, y, z, w = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    one, two = dtype(1.0), dtype(2.0)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=dtype)


def project(kpix, mu, K, T7, K_dst, dst_size, dtype=np.float64):
    """The header's projection, step by step in `dtype` (np.longdouble: the yardstick).  kpix: the slot's pixels; mu: the seeds' fp64
    mu or the fp32 plane widened; K, K_dst: (fx, fy, cx, cy); T7: (p, q_xyzw) of T_dst_src; dst_size: (dst_H, dst_W).
    Returns dict(px, py, idp: every point's; Zp; keep: mask; xy, idp_kept, src: the kept points in order)"""
    kp = np.asarray(kpix, dtype=np.float64).astype(dtype)
    mu = np.asarray(mu, dtype=np.float64).astype(dtype)
    fx, fy, cx, cy = [dtype(v) for v in K]
    fxd, fyd, cxd, cyd = [dtype(v) for v in K_dst]
    T7 = np.asarray(T7, dtype=np.float64)
    R, t = quat_to_R(T7[3:7], dtype), T7[:3].astype(dtype)
    u, v = kp[:, 0], kp[:, 1]
    d = dtype(1.0) / mu
    X, Y, Z = d * ((u - cx) / fx), d * ((v - cy) / fy), d
    Xp = ((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]
    Yp = ((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]
    Zp = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        px, py, idp = fxd * (Xp / Zp) + cxd, fyd * (Yp / Zp) + cyd, dtype(1.0) / Zp
    dH, dW = dst_size
    keep = (px >= 0) & (px < dW) & (py >= 0) & (py < dH)
    return dict(px=px, py=py, idp=idp, Zp=Zp, keep=keep, xy=np.column_stack([px, py])[keep], idp_kept=idp[keep],
                src=np.flatnonzero(keep).astype(np.int32))
