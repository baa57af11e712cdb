"""numpy restatement of the reference's KLT point trackers: Tracker::trackPoints / trackPointsPyr (src/tracking/Tracker.cpp:378-488)
after their getCoord(true) call, i.e. fed the warped coordinates that call returned:

  2. drawValuesPoints (Utils.cpp:124-193), "bilinear", over the double values, then cv::GaussianBlur 3 x 3, sigma 0.5
  3. splitImageInPatches (Utils.cpp:608-633): copyMakeBorder by r, reflect-101, and cv::Rect at the TRUNCATED coordinates
  4. kltTracker (Utils.cpp:735-759): five cv::sums of element-wise products, f = -M^-1 b with Eigen's 2 x 2 inverse
  5. trackPointsPyr: pyramidPatches (Utils.cpp:662-673) and f += klt_j / 2^j / 2^j from the coarsest level down

Every step is restated literally and in the reference's order where it has one: the splat adds each point's four corners in point
order, cv::sum runs over the flattened product matrix four terms at a time.

pyrDown is OUR READING of OpenCV's cv::pyrDown (OpenCV is not available here to check it against): the 5 x 5 kernel
[1 4 6 4 1]^2 / 256, horizontally c*6 + (l1 + r1)*4 + l2 + r2, then the same vertically, times 1/256, with reflect-101 at the
borders of the patch itself — it does not look outside the ROI.  The device shares this assumption, so parity cannot catch it if it
is wrong.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from np_frame_oracle import gaussian_blur_3x3  # noqa: E402


def pyr_radius(num_level):
    """uint16_t patch_radius = 3 * 2^(L-1) + L; patch_radius /= 2 (Tracker.cpp:440-441)"""
    r = np.uint16(3 * 2.0 ** (num_level - 1) + num_level)
    return int(r // 2)


def border_interpolate(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), elementwise, repeating while p is outside"""
    p = np.array(p, dtype=np.int64, copy=True)
    if n == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p = np.where(lo, -p, p)
        p = np.where(hi, 2 * n - 2 - p, p)


def draw_values_points(coord, values, H, W, s=0.5):
    """drawValuesPoints(points, values, H, W, "bilinear", s): the four corner weights (0 for a corner outside the image), the
    corner indices clipped, contributions added point by point; then GaussianBlur 3 x 3 with sigma s (KeyFrame.hpp:181,185)."""
    x, y = np.asarray(coord, dtype=np.float64)[:, 0], np.asarray(coord, dtype=np.float64)[:, 1]
    v = np.asarray(values, dtype=np.float64)
    img = np.zeros((H, W))
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1

    def inside(xx, yy):
        return (xx < W) & (yy < H) & (xx >= 0) & (yy >= 0)

    wa = np.where(inside(x0, y0), (x1 - x) * (y1 - y), 0.0)
    wb = np.where(inside(x0, y1), (x1 - x) * (y - y0), 0.0)
    wc = np.where(inside(x1, y0), (x - x0) * (y1 - y), 0.0)
    wd = np.where(inside(x1, y1), (x - x0) * (y - y0), 0.0)
    cx0, cx1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)
    cy0, cy1 = np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
    # one unbuffered add in the order (point, corner a, b, c, d): each pixel sums in point order
    rows = np.stack([cy0, cy1, cy0, cy1], axis=1).ravel()
    cols = np.stack([cx0, cx0, cx1, cx1], axis=1).ravel()
    vals = np.stack([wa * v, wb * v, wc * v, wd * v], axis=1).ravel()
    np.add.at(img, (rows, cols), vals)
    if s > 0:
        img = gaussian_blur_3x3(img, s)
    return img


def split_image_in_patches(img, coord, r):
    """N x (2r+1) x (2r+1): copyMakeBorder(img, r, r, r, r, BORDER_DEFAULT) then img(Rect(p.x, p.y, 2r+1, 2r+1)) with the double
    coordinates truncated to int.  (The reference throws when the rectangle leaves the padded image — x == cols or y == rows; the
    reflection simply continues here, as on the device.)"""
    H, W = img.shape
    c = np.asarray(coord, dtype=np.float64)
    tx, ty = np.trunc(c[:, 0]).astype(np.int64), np.trunc(c[:, 1]).astype(np.int64)
    k = np.arange(2 * r + 1)
    cols = border_interpolate(tx[:, None] - r + k[None, :], W)
    rows = border_interpolate(ty[:, None] - r + k[None, :], H)
    return img[rows[:, :, None], cols[:, None, :]]


def pyr_down(p, size):
    """cv::pyrDown(p, out, Size(size, size)) of a stack of square patches (N x s x s), reflect-101 inside the patch"""
    s = p.shape[-1]
    t = np.arange(size)
    c = [border_interpolate(2 * t + u - 2, s) for u in range(5)]
    h = p[:, :, c[2]] * 6 + (p[:, :, c[1]] + p[:, :, c[3]]) * 4 + p[:, :, c[0]] + p[:, :, c[4]]
    v = h[:, c[2], :] * 6 + (h[:, c[1], :] + h[:, c[3], :]) * 4 + h[:, c[0], :] + h[:, c[4], :]
    return v * (1.0 / 256)


def pyramid_patches(p, num_level):
    """pyramidPatches: level i = pyrDown of level i-1 to the ORIGINAL size / 2^i (15 -> 7 -> 3 for L = 3)"""
    out = [p]
    s = p.shape[-1]
    for i in range(1, num_level):
        out.append(pyr_down(out[-1], s // 2 ** i))
    return out


def cv_sum(m):
    """cv::sum of a continuous CV_64F matrix per patch: s += ((a + b) + c) + d over the flattened elements, then the rest one by one"""
    m = m.reshape(m.shape[0], -1)
    n = m.shape[1]
    s = np.zeros(m.shape[0])
    q = 0
    while q + 4 <= n:
        s = s + (((m[:, q] + m[:, q + 1]) + m[:, q + 2]) + m[:, q + 3])
        q += 4
    while q < n:
        s = s + m[:, q]
        q += 1
    return s


def klt_tracker(px, py, pe):
    """kltTracker per patch: M = [[Ixx, Ixy], [Ixy, Iyy]], b = [Ixt, Iyt], -M.inverse() * b (Eigen: invdet = 1 / det)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        sxx, syy, sxy = cv_sum(px * px), cv_sum(py * py), cv_sum(px * py)
        sxt, syt = cv_sum(px * pe), cv_sum(py * pe)
        det = sxx * syy - sxy * sxy
        invdet = 1.0 / det
        i00, i10, i01, i11 = syy * invdet, -sxy * invdet, -sxy * invdet, sxx * invdet
        f0 = -i00 * sxt + -i01 * syt
        f1 = -i10 * sxt + -i11 * syt
    return np.column_stack([f0, f1]), np.stack([sxx, syy, sxy], axis=1)


def _patches(coord, grad, frame, r):
    H, W = frame.shape
    g = np.asarray(grad, dtype=np.float64)
    gx = draw_values_points(coord, g[:, 0], H, W)
    gy = draw_values_points(coord, g[:, 1], H, W)
    return (split_image_in_patches(gx, coord, r), split_image_in_patches(gy, coord, r),
            split_image_in_patches(np.asarray(frame, dtype=np.float64), coord, r))


def cond(m):
    """condition number of each M (rows sxx, syy, sxy) in the 2-norm"""
    sxx, syy, sxy = m[:, 0], m[:, 1], m[:, 2]
    tr, dt = sxx + syy, sxx * syy - sxy * sxy
    disc = np.sqrt(np.maximum(tr * tr / 4 - dt, 0.0))
    lmax, lmin = tr / 2 + disc, tr / 2 - disc
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lmin > 0, lmax / lmin, np.inf)


def track_points(coord, grad, frame, patch_radius=7):
    """trackPoints' flow of every point (steps 2-4): returns (flow N x 2, M entries N x 3)"""
    px, py, pe = _patches(coord, grad, frame, patch_radius)
    return klt_tracker(px, py, pe)


def track_points_pyr(coord, grad, frame, num_level=3):
    """trackPointsPyr's f of every point: sum over j = L-1 .. 0 of (1/scale) * klt_j / scale.  Returns (f N x 2, M of every level)"""
    px, py, pe = _patches(coord, grad, frame, pyr_radius(num_level))
    lx, ly, le = pyramid_patches(px, num_level), pyramid_patches(py, num_level), pyramid_patches(pe, num_level)
    f = np.zeros((px.shape[0], 2))
    ms = []
    for j in range(num_level - 1, -1, -1):
        scale = 2.0 ** j
        k, m = klt_tracker(lx[j], ly[j], le[j])
        f = f + (1.0 / scale) * k / scale
        ms.append(m)
    return f, ms
