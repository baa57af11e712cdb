"""numpy restatement of the reference's epiline tracker, Tracker::trackPointsAlongEpiline (src/tracking/Tracker.cpp:490-553), as
include/eds_hip_epiline.h states it:

  1. getModel(v, w, "bilinear") (KeyFrame.cpp:1358-1423): per point f = compute_flow(norm_coord, v, w, mu) (Utils.hpp:165-173),
     m = -(g . f) / sqrt(1e-3 + sum m^2), splatted bilinearly in point order and blurred 3 x 3 with sigma 0.5 (np_klt_oracle)
  2. splitImageInPatches (Utils.cpp:608-633): copyMakeBorder by r, cv::Rect at the TRUNCATED pixel, each patch in fp32
  3. copyMakeBorder(event_frame, r) in fp32
  4. matchTemplate twice: p_ssd = the first minimum of TM_SQDIFF_NORMED, p_ncc = the first maximum of TM_CCORR_NORMED
  5. the cull |‖p_ssd‖ - ‖p_ncc‖| > 5

The normed-score rule is OUR READING of OpenCV's common_matchTemplate (OpenCV is not available here to check it against), with
E = sum P^2 over the window, S = sum T^2, C = sum P T and t = sqrt(E) sqrt(S):
  CCORR_NORMED   C / t if |C| < t, +-1 if |C| < 1.125 t, else 0
  SQDIFF_NORMED  num = max(E - 2C + S, 0); num / t if num < t, else 1
Scores are rounded to fp32 (OpenCV's CV_32F result) before they are compared, and the first position in row-major order wins a tie
(cv::minMaxLoc).  The device shares this reading, so parity cannot catch it if it is wrong.  Here C, E and S are fp64 sums of exact
fp32 products; the device accumulates C in fp32.

Not reproduced, as on the device: the rectangles the reference's matchTemplate draws into its (shallow-copied) search image, the
cv::normalize(NORM_MINMAX) before minMaxLoc, the prints and PNG writes.
"""
import numpy as np

import np_klt_oracle as ko

BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101 = 0, 1, 2, 4


def tol(r):
    """the score tolerance of fp32 accumulation: 2 K 2^-24 + 2^-23 with K = (2r + 1)^2 (|dC| <= gamma_K t, Cauchy-Schwarz)"""
    K = (2 * r + 1) ** 2
    return 2.0 * K * 2.0 ** -24 + 2.0 ** -23


def slot_pixels(norm_xy, fx, fy, cx, cy):
    """the keyframe pixel as a tracker slot holds it: u = fx x + cx in fp64, split into floor(u) and an fp32 fraction"""
    n = np.asarray(norm_xy, dtype=np.float64)
    out = np.empty_like(n)
    for c, (f, cc) in enumerate(((fx, cx), (fy, cy))):
        u = f * n[:, c] + cc
        cu = np.clip(np.floor(u), -32000.0, 32000.0)
        out[:, c] = cu + (u - cu).astype(np.float32).astype(np.float64)
    return out


def border_index(p, n, border):
    """cv::borderInterpolate(p, n, border) elementwise for REPLICATE, REFLECT, REFLECT_101 (repeated while p is outside)"""
    p = np.array(p, dtype=np.int64, copy=True)
    if border == BORDER_REPLICATE:
        return np.clip(p, 0, n - 1)
    if n == 1:
        return np.zeros_like(p)
    delta = 1 if border == BORDER_REFLECT_101 else 0
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p - 1 + delta, p)
        p = np.where(hi, n - 1 - (p - n) - delta, p)


def take_bordered(img, rows, cols, border, value):
    """img at the integer positions (rows[..., :, None], cols[..., None, :]), extrapolated as copyMakeBorder does"""
    H, W = img.shape
    rows, cols = np.asarray(rows), np.asarray(cols)
    if border == BORDER_CONSTANT:
        rr, cc = np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)
        out = img[rr[..., :, None], cc[..., None, :]].astype(np.float64)
        inside = ((rows >= 0) & (rows < H))[..., :, None] & ((cols >= 0) & (cols < W))[..., None, :]
        return np.where(inside, out, float(value))
    return img[border_index(rows, H, border)[..., :, None], border_index(cols, W, border)[..., None, :]]


def copy_make_border(img, r, border, value):
    H, W = img.shape
    return take_bordered(np.asarray(img), np.arange(-r, H + r), np.arange(-r, W + r), border, value)


def sparse_model(kpix, grad, idp, vel, K):
    """getSparseModel: the normalised model value of every point (fp64, no FMA, the norm summed in point order)"""
    fx, fy, cx, cy = K
    kp = np.asarray(kpix, dtype=np.float64)
    g = np.asarray(grad, dtype=np.float64)
    mu = np.asarray(idp, dtype=np.float64)
    v0, v1, v2, w0, w1, w2 = [float(a) for a in vel]
    xp, yp = (kp[:, 0] - cx) / fx, (kp[:, 1] - cy) / fy
    f0 = (-mu * v0) + ((xp * mu) * v2) + ((xp * yp) * w0) - (1.0 + xp * xp) * w1 + (yp * w2)
    f1 = (-mu * v1) + ((yp * mu) * v2) + (1.0 + yp * yp) * w0 - ((xp * yp) * w1) - (xp * w2)
    m = -(g[:, 0] * f0 + g[:, 1] * f1)
    acc = 1e-03
    for sq in (m * m).tolist():
        acc += sq
    return m / np.sqrt(acc)


def model_image(kpix, grad, idp, vel, K, H, W):
    """getModel(v, w, "bilinear", 0.5): H x W fp64"""
    return ko.draw_values_points(kpix, sparse_model(kpix, grad, idp, vel, K), H, W, 0.5)


def templates(model, kpix, r, border, value):
    """N x (2r+1) x (2r+1) fp32 patches of the padded model at the truncated keyframe pixels"""
    kp = np.asarray(kpix, dtype=np.float64)
    tx, ty = np.trunc(kp[:, 0]).astype(np.int64), np.trunc(kp[:, 1]).astype(np.int64)
    k = np.arange(2 * r + 1)
    return take_bordered(model, ty[:, None] - r + k[None, :], tx[:, None] - r + k[None, :], border, value).astype(np.float32)


def normed_scores(C, E, S):
    """(ssd, ncc) as fp32 from fp64 C, E, S by the clamp rule"""
    C, E, S = np.asarray(C, np.float64), np.asarray(E, np.float64), np.asarray(S, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = np.sqrt(np.where(E < 0, 0.0, E)) * np.sqrt(S)
        aC = np.abs(C)
        ncc = np.where(aC < t, C / t, np.where(aC < 1.125 * t, np.where(C > 0, 1.0, -1.0), 0.0))
        num = E - 2.0 * C + S
        num = np.where(num < 0, 0.0, num)
        ssd = np.where(num < t, num / t, 1.0)
    return ssd.astype(np.float32), ncc.astype(np.float32)


def score_maps(padded, tmpl, rows_per_chunk=32):
    """the two H x W fp32 score maps of every template, (n, H, W) each.  padded: the fp32 search image padded by r"""
    P = np.asarray(padded, dtype=np.float32).astype(np.float64)
    T = np.asarray(tmpl, dtype=np.float32).astype(np.float64)
    n, S = T.shape[0], T.shape[1]
    H, W = P.shape[0] - S + 1, P.shape[1] - S + 1
    Tm = T.reshape(n, S * S)
    Ssum = (Tm * Tm).sum(axis=1)
    ssd, ncc = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.float32)
    for y0 in range(0, H, rows_per_chunk):
        y1 = min(H, y0 + rows_per_chunk)
        win = np.lib.stride_tricks.sliding_window_view(P[y0:y1 + S - 1], (S, S)).reshape(y1 - y0, W, S * S)
        E = (win * win).sum(axis=2)
        C = np.einsum("hwk,nk->nhw", win, Tm, optimize=True)
        s, c = normed_scores(C, E[None], Ssum[:, None, None])
        ssd[:, y0:y1], ncc[:, y0:y1] = s, c
    return ssd, ncc


def arg_best(m, largest):
    """first row-major position of the extremum of an fp32 map among its finite values, ((x, y), score); (-1, -1) when none is"""
    f = m.ravel().astype(np.float64)
    ok = np.isfinite(f)
    if not ok.any():
        return (-1, -1), np.nan
    f = np.where(ok, f, -np.inf if largest else np.inf)
    i = int(np.argmax(f) if largest else np.argmin(f))
    return (i % m.shape[1], i // m.shape[1]), float(m.ravel()[i])


def cull(ssd_xy, ncc_xy):
    """True where the reference keeps the point: |‖p_ssd‖ - ‖p_ncc‖| <= 5, and both methods found a finite score"""
    s, n = np.asarray(ssd_xy, np.float64), np.asarray(ncc_xy, np.float64)
    d = np.abs(np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) - np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]))
    return (d <= 5.0) & (s[:, 0] >= 0) & (n[:, 0] >= 0)


def match(frame, tmpl, r, border, value, with_maps=False):
    """both matchTemplate calls of every template against the padded fp32 frame"""
    padded = copy_make_border(np.asarray(frame, dtype=np.float32).astype(np.float64), r, border, value).astype(np.float32)
    ssd_m, ncc_m = score_maps(padded, tmpl)
    n = tmpl.shape[0]
    ssd_xy, ncc_xy = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
    s_ssd, s_ncc = np.zeros(n), np.zeros(n)
    for i in range(n):
        ssd_xy[i], s_ssd[i] = arg_best(ssd_m[i], False)
        ncc_xy[i], s_ncc[i] = arg_best(ncc_m[i], True)
    out = dict(ssd=ssd_xy, ncc=ncc_xy, s_ssd=s_ssd, s_ncc=s_ncc, keep=cull(ssd_xy, ncc_xy))
    if with_maps:
        out.update(ssd_map=ssd_m, ncc_map=ncc_m)
    return out


def track_points_along_epiline(kpix, grad, idp, vel, K, frame, r=7, border=BORDER_REFLECT_101, value=255, sample=None, with_maps=False):
    """the whole call for the points `sample` (default: all): dict(ssd, ncc, s_ssd, s_ncc, keep[, ssd_map, ncc_map], model)"""
    H, W = np.asarray(frame).shape
    model = model_image(kpix, grad, idp, vel, K, H, W)
    kp = np.asarray(kpix, dtype=np.float64)
    idx = np.arange(len(kp)) if sample is None else np.asarray(sample)
    out = match(frame, templates(model, kp[idx], r, border, value), r, border, value, with_maps)
    out["model"] = model
    return out
