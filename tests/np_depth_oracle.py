"""CPU oracle of eds::mapping::DepthPoints (reference src/mapping/DepthPoints.{hpp,cpp}, src/utils/Utils.hpp:272-345): a literal
numpy restatement, branch by branch, for the device filter of include/eds_hip_depth.h.

Two forms of the same arithmetic:
  * per point (`inv_depth_two_points_eucl`, `compute_tau`, `filter_vogiatzis`): the reference's cv::Mat code with P_kf / P_ef
    as matrices and np.linalg.pinv where it calls inv(DECOMP_SVD);
  * vectorised (`update`): the same operations in the same order over arrays, for thousands of alignments.
Quaternions are x, y, z, w; a pose (p, q) maps keyframe points into the event frame (the tracker's state is T_ef_kf).
"""
from __future__ import annotations

import math

import numpy as np

PX_NOISE = 3.0


def quat_to_R(q):
    """Eigen's toRotationMatrix (no normalisation), as csrc/eds_math.hpp quat_to_R"""
    x, y, z, w = [float(v) for v in q]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def quat_to_RmI(q):
    x, y, z, w = [float(v) for v in q]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[-(tyy + tzz), txy - twz, txz + twy], [txy + twz, -(txx + tzz), tyz - twx], [txz - twy, tyz + twx, -(txx + tyy)]])


def K_matrix(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


class Params:
    """DepthPoints' scalars after init (DepthPoints.cpp:59-99)"""

    def __init__(self, K, min_depth, max_depth, threshold=100.0, init_a=2.0, init_b=5.0):
        self.K = np.asarray(K, dtype=np.float64)
        self.fx, self.fy, self.cx, self.cy = self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2]
        self.mu_range = max_depth - min_depth
        self.px_error_angle = math.atan(PX_NOISE / (2.0 * self.fx)) + math.atan(PX_NOISE / (2.0 * self.fy))    # getAngleError
        self.seed_mu_range = 1.0 / min_depth          # computed and never used by the reference
        self.convergence_sigma2_thresh = threshold
        self.min_depth, self.max_depth, self.init_a, self.init_b = min_depth, max_depth, init_a, init_b


def init_constant(prm: Params, num_points):
    """init(K, num_points, ...): mu = 1/((max-min)/2), sigma2 = mu_range^2"""
    v = np.array([1.0 / ((prm.max_depth - prm.min_depth) / 2.0), prm.mu_range * prm.mu_range, prm.init_a, prm.init_b])
    return np.tile(v, (num_points, 1))


def init_vector(prm: Params, inv_depth):
    """init(K, inv_depth, ...): mu = idp, sigma2 = mu_range^2/36"""
    inv_depth = np.asarray(inv_depth, dtype=np.float64)
    s = np.empty((len(inv_depth), 4))
    s[:, 0] = inv_depth
    s[:, 1] = (prm.mu_range * prm.mu_range) / 36.0
    s[:, 2] = prm.init_a
    s[:, 3] = prm.init_b
    return s


def T_ef_kf_from(T_kf_ef=None, p=None, q=None):
    """(R, t) of T_ef_kf: the inverse of T_kf_ef = (p', q') given as a pair, or the tracker's own (p, q)"""
    if T_kf_ef is not None:
        pk, qk = np.asarray(T_kf_ef[0], dtype=np.float64), T_kf_ef[1]
        R = quat_to_R(qk).T
        t = -np.array([R[r, 0] * pk[0] + R[r, 1] * pk[1] + R[r, 2] * pk[2] for r in range(3)])
        return R, t, pk.copy()
    R = quat_to_R(q)
    t = np.asarray(p, dtype=np.float64).copy()
    t_kf_ef = -np.array([R[0, r] * t[0] + R[1, r] * t[1] + R[2, r] * t[2] for r in range(3)])
    return R, t, t_kf_ef


def projection_matrices(K, R, t):
    """P_kf = K [I | 0], P_ef = K T_ef_kf[0:3] (DepthPoints.cpp:143-148)"""
    P_kf = np.hstack([K, np.zeros((3, 1))])
    P_ef = K @ np.hstack([R, np.asarray(t).reshape(3, 1)])
    return P_kf, P_ef


def closed_form_K_inverse(K):
    """K^-1 as the device's host code and `update` form it: entry by entry, no SVD"""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])


def _rows_times(M, x):
    """M x, each row summed left to right (no BLAS: its order and contraction are not ours to know)"""
    return np.array([M[r, 0] * x[0] + M[r, 1] * x[1] + M[r, 2] * x[2] for r in range(3)])


def inv_depth_two_points_eucl(x1, x2, P1, P2, inv_M1=None):
    """invDepthTwoPointsEucl (DepthPoints.cpp:368-397), literally: homogeneous 3-vectors x1 (keyframe), x2 (event frame).
    inv_M1: the inverse to use in place of pinv(M1) — with `closed_form_K_inverse` and row-wise products the triangulation rounds as
    `update`'s does, to the last bit (what decides skip against update where the exact inverse depth is 0)"""
    M1, M2 = P1[:, :3], P2[:, :3]
    if inv_M1 is not None:
        x1p = _rows_times(M2, _rows_times(inv_M1, x1))
        e2 = P2[:, 3]                               # C1 = (0, 0, 0, 1): P1's last column is zero
        aux1 = np.array([x1p[1] * x2[2] - x1p[2] * x2[1], x1p[2] * x2[0] - x1p[0] * x2[2], x1p[0] * x2[1] - x1p[1] * x2[0]])
        aux2 = np.array([x2[1] * e2[2] - x2[2] * e2[1], x2[2] * e2[0] - x2[0] * e2[2], x2[0] * e2[1] - x2[1] * e2[0]])
        with np.errstate(all="ignore"):
            return float((aux1[0] * aux2[0] + aux1[1] * aux2[1] + aux1[2] * aux2[2]) / (aux2[0] * aux2[0] + aux2[1] * aux2[1] + aux2[2] * aux2[2]))
    invM1 = np.linalg.pinv(M1)
    C1 = np.ones(4)
    C1[:3] = -invM1 @ P1[:, 3]
    e2 = P2 @ C1
    x1p = M2 @ (invM1 @ x1)
    aux1 = np.cross(x1p, x2)
    aux2 = np.cross(x2, e2)
    return float(np.dot(aux1, aux2) / np.dot(aux2, aux2))


def inv_depth_closed_form(K, R, t, x_kf, x_ef):
    """a = K R K^-1 x_kf, e = K t, inv = ((a x x_ef).(x_ef x e)) / |x_ef x e|^2"""
    a = K @ R @ np.linalg.inv(K) @ x_kf
    e = K @ t
    c = np.cross(x_ef, e)
    return float(np.dot(np.cross(a, x_ef), c) / np.dot(c, c))


def compute_tau(t_kf_ef, x_norm, z, px_error_angle):
    """computeTau (DepthPoints.hpp:165-182): t of T_kf_ef, bearing of the event-frame pixel"""
    t = np.asarray(t_kf_ef, dtype=np.float64)
    xb = np.array([x_norm[0], x_norm[1], 1.0])
    xb = xb / math.sqrt(xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2])
    a = xb * z - t
    t_norm = math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    a_norm = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    alpha = _acos((xb[0] * t[0] + xb[1] * t[1] + xb[2] * t[2]) / t_norm)
    beta = _acos((a[0] * -t[0] + a[1] * -t[1] + a[2] * -t[2]) / (t_norm * a_norm))
    beta_plus = beta + px_error_angle
    gamma_plus = math.pi - alpha - beta_plus
    z_plus = t_norm * math.sin(beta_plus) / math.sin(gamma_plus)
    return z_plus - z


def _acos(x):
    return math.acos(x) if -1.0 <= x <= 1.0 else float("nan")


def sigma2_from_depth_sigma(depth, depth_sigma):
    """getSigma2FromDepthSigma (DepthPoints.hpp:184-189); std::max(1e-12, d) is (1e-12 < d) ? d : 1e-12 (NaN -> 1e-12)"""
    d = depth - depth_sigma
    with np.errstate(all="ignore"):                 # IEEE division: 1 / 0 is inf, as in C++ (a Python float raises)
        sigma = 0.5 * (1.0 / (d if 1e-12 < d else 1e-12) - float(np.float64(1.0) / np.float64(depth + depth_sigma)))
    return sigma * sigma


def norm_pdf(x, mean, sigma):
    """Utils.hpp:337-345"""
    exponent = x - mean
    exponent *= -exponent
    exponent /= 2 * sigma * sigma
    result = math.exp(exponent)
    result /= sigma * math.sqrt(2 * math.pi)
    return result


def filter_vogiatzis(z, tau2, mu_range, state):
    """filterVogiatzis (DepthPoints.cpp:180-228) on state = [mu, sigma2, a, b] in place; returns (ran, sigma2_restored, mu_reset)"""
    mu, sigma2, a, b = [float(v) for v in state]
    norm_scale = math.sqrt(sigma2 + tau2) if sigma2 + tau2 >= 0 else float("nan")
    if math.isnan(norm_scale):
        return False, False, False
    oldsigma2 = sigma2
    s2 = 1.0 / (1.0 / sigma2 + 1.0 / tau2)
    m = s2 * (mu / sigma2 + z / tau2)
    uniform_x = 1.0 / mu_range
    C1 = a / (a + b) * norm_pdf(z, mu, norm_scale)
    C2 = b / (a + b) * uniform_x
    normalization_constant = C1 + C2
    C1 /= normalization_constant
    C2 /= normalization_constant
    f = C1 * (a + 1.0) / (a + b + 1.0) + C2 * a / (a + b + 1.0)
    e = C1 * (a + 1.0) * (a + 2.0) / ((a + b + 1.0) * (a + b + 2.0)) + C2 * a * (a + 1.0) / ((a + b + 1.0) * (a + b + 2.0))
    mu_new = C1 * m + C2 * mu
    sigma2 = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu_new * mu_new
    mu = mu_new
    a = (e - f) / (f - e / f)
    b = a * (1.0 - f) / f
    restored = reset = False
    if sigma2 < 0.0:
        sigma2 = oldsigma2
        restored = True
    if mu < 0.0:
        mu = 1.0
        reset = True
    state[:] = (mu, sigma2, a, b)
    return True, restored, reset


def is_converged(state, mu_range, threshold):
    thresh = mu_range / threshold
    return state[1] < thresh * thresh


def update_literal(prm: Params, seeds, kf_coord, ef_coord, R, t, t_kf_ef, closed_form_inverse=False):
    """DepthPoints::update (ef_coord overload, DepthPoints.cpp:101-135), one point at a time; seeds N x 4 in place.
    Returns the summary counts.  closed_form_inverse: K^-1 and P_ef entry by entry as `update` forms them, instead of pinv and BLAS."""
    P_kf, P_ef = projection_matrices(prm.K, R, t)
    inv_M1 = None
    if closed_form_inverse:
        P_ef, inv_M1 = projection_rows(prm.K, R, t), closed_form_K_inverse(prm.K)
    cnt = dict(updated=0, skipped_nan=0, sigma2_restored=0, mu_reset=0, converged=0)
    for i in range(len(seeds)):
        x_kf = np.array([kf_coord[i][0], kf_coord[i][1], 1.0])
        x_ef = np.array([ef_coord[i][0], ef_coord[i][1], 1.0])
        with np.errstate(all="ignore"):
            inv_depth = inv_depth_two_points_eucl(x_kf, x_ef, P_kf, P_ef, inv_M1)
            depth = 1.0 / inv_depth if inv_depth != 0 else math.copysign(math.inf, inv_depth)
            x_norm = ((x_ef[0] - prm.cx) / prm.fx, (x_ef[1] - prm.cy) / prm.fy)
            try:
                tau = compute_tau(t_kf_ef, x_norm, depth, prm.px_error_angle)
            except (ValueError, ZeroDivisionError, OverflowError):
                tau = float("nan")
            tau2 = sigma2_from_depth_sigma(depth, tau)
        ran, restored, reset = filter_vogiatzis(inv_depth, tau2, prm.mu_range, seeds[i])
        cnt["updated"] += ran
        cnt["skipped_nan"] += not ran
        cnt["sigma2_restored"] += restored
        cnt["mu_reset"] += reset
        cnt["converged"] += bool(is_converged(seeds[i], prm.mu_range, prm.convergence_sigma2_thresh))
    return cnt


# ---- vectorised: the same operations in the same order over arrays ------------------------------------------------------------
def projection_rows(K, R, t, T=np.float64):
    """P_ef = K [R | t] with the products and sums in the order the device's host code forms them (csrc/eds_depth.hip)"""
    K, R, t = np.asarray(K, dtype=T), np.asarray(R, dtype=T), np.asarray(t, dtype=T)
    Pe = np.empty((3, 4), dtype=T)
    for r in range(3):
        for c in range(3):
            Pe[r, c] = K[r, 0] * R[0, c] + K[r, 1] * R[1, c] + K[r, 2] * R[2, c]
        Pe[r, 3] = K[r, 0] * t[0] + K[r, 1] * t[1] + K[r, 2] * t[2]
    return Pe


def evaluate(prm: Params, seeds, kf_coord, ef_coord, R, t, t_kf_ef, T=np.float64):
    """DepthPoints::update per point, nothing written: every operation of `update` in its order, in the number format T.  The inputs
    (fp64 pixels, seeds, K, R, t, px_error_angle and the reference's fp64 constant pi) are the same numbers in every format;
    T = np.longdouble is the extended-precision evaluation of the same formulas.  Returns a dict of length-N arrays:
      run                          filterVogiatzis ran (not the NaN skip)
      restored, reset, converged   the branches taken, and isConverged of the seed the point ends with
      mu_new, sigma2_new           BEFORE the sigma2 < 0 / mu < 0 branches
      a_new, b_new, m, C1, C2      the other updated values and the terms of mu_new = C1 m + C2 mu
      f, e, inv_depth, tau2        the Beta moments behind a_new / b_new, the triangulated inverse depth and its variance
      seeds                        N x 4, the seeds after the update (input rows where run is False)"""
    with np.errstate(all="ignore"):
        c = lambda x: np.asarray(x, dtype=T)
        one, two, half = T(1.0), T(2.0), T(0.5)
        fx, fy, cx, cy = T(prm.fx), T(prm.fy), T(prm.cx), T(prm.cy)
        pi = T(math.pi)
        zero = T(0.0)
        Ki = [[one / fx, zero, -cx / fx], [zero, one / fy, -cy / fy], [zero, zero, one]]
        Pe = projection_rows(prm.K, R, t, T)
        kf_coord, ef_coord, seeds = c(kf_coord), c(ef_coord), c(seeds)
        u, v = kf_coord[:, 0], kf_coord[:, 1]
        ue, ve = ef_coord[:, 0], ef_coord[:, 1]
        y0 = Ki[0][0] * u + Ki[0][1] * v + Ki[0][2]
        y1 = Ki[1][0] * u + Ki[1][1] * v + Ki[1][2]
        y2 = Ki[2][0] * u + Ki[2][1] * v + Ki[2][2]
        p0 = Pe[0, 0] * y0 + Pe[0, 1] * y1 + Pe[0, 2] * y2
        p1 = Pe[1, 0] * y0 + Pe[1, 1] * y1 + Pe[1, 2] * y2
        p2 = Pe[2, 0] * y0 + Pe[2, 1] * y1 + Pe[2, 2] * y2
        e0, e1, e2 = Pe[0, 3], Pe[1, 3], Pe[2, 3]
        a1x, a1y, a1z = p1 * one - p2 * ve, p2 * ue - p0 * one, p0 * ve - p1 * ue
        a2x, a2y, a2z = ve * e2 - one * e1, one * e0 - ue * e2, ue * e1 - ve * e0
        inv_depth = (a1x * a2x + a1y * a2y + a1z * a2z) / (a2x * a2x + a2y * a2y + a2z * a2z)
        depth = one / inv_depth
        xn, yn = (ue - cx) / fx, (ve - cy) / fy
        bn = np.sqrt(xn * xn + yn * yn + one * one)
        bx, by, bz = xn / bn, yn / bn, one / bn
        tx, ty, tz = (T(x) for x in t_kf_ef)
        ax, ay, az = bx * depth - tx, by * depth - ty, bz * depth - tz
        t_norm = np.sqrt(tx * tx + ty * ty + tz * tz)
        a_norm = np.sqrt(ax * ax + ay * ay + az * az)
        alpha = np.arccos((bx * tx + by * ty + bz * tz) / t_norm)
        beta = np.arccos((ax * -tx + ay * -ty + az * -tz) / (t_norm * a_norm))
        beta_plus = beta + T(prm.px_error_angle)
        gamma_plus = pi - alpha - beta_plus
        z_plus = t_norm * np.sin(beta_plus) / np.sin(gamma_plus)
        tau = z_plus - depth
        dm = depth - tau
        sg = half * (one / np.where(T(1e-12) < dm, dm, T(1e-12)) - one / (depth + tau))
        tau2 = sg * sg
        mu, sigma2, a, b = (seeds[:, k].copy() for k in range(4))
        norm_scale = np.sqrt(sigma2 + tau2)
        run = ~np.isnan(norm_scale)
        z = inv_depth
        s2 = one / (one / sigma2 + one / tau2)
        m = s2 * (mu / sigma2 + z / tau2)
        uniform_x = one / T(prm.mu_range)
        ex = z - mu
        ex = ex * -ex
        ex = ex / (two * norm_scale * norm_scale)
        pdf = np.exp(ex) / (norm_scale * np.sqrt(two * pi))
        C1 = a / (a + b) * pdf
        C2 = b / (a + b) * uniform_x
        nc = C1 + C2
        C1 = C1 / nc
        C2 = C2 / nc
        f = C1 * (a + one) / (a + b + one) + C2 * a / (a + b + one)
        e = C1 * (a + one) * (a + two) / ((a + b + one) * (a + b + two)) + C2 * a * (a + one) / ((a + b + one) * (a + b + two))
        mu_new = C1 * m + C2 * mu
        sigma2_new = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu_new * mu_new
        a_new = (e - f) / (f - e / f)
        b_new = a_new * (one - f) / f
        restored = run & (sigma2_new < zero)
        reset = run & (mu_new < zero)
        out = seeds.copy()
        out[run, 0] = np.where(mu_new < zero, one, mu_new)[run]
        out[run, 1] = np.where(sigma2_new < zero, sigma2, sigma2_new)[run]
        out[run, 2], out[run, 3] = a_new[run], b_new[run]
        th = T(prm.mu_range) / T(prm.convergence_sigma2_thresh)
        conv = out[:, 1] < th * th
    return dict(run=run, restored=restored, reset=reset, converged=conv, mu_new=mu_new, sigma2_new=sigma2_new, a_new=a_new, b_new=b_new,
                m=m, C1=C1, C2=C2, f=f, e=e, seeds=out, inv_depth=inv_depth, tau2=tau2, thresh2=th * th)


def update(prm: Params, seeds, kf_coord, ef_coord, R, t, t_kf_ef):
    """seeds N x 4 (updated in place), kf_coord / ef_coord N x 2 pixels.  Returns the summary counts."""
    ev = evaluate(prm, seeds, np.asarray(kf_coord, dtype=np.float64), np.asarray(ef_coord, dtype=np.float64), R, t, t_kf_ef)
    seeds[:] = ev["seeds"]
    return summary_of(ev)


def summary_of(ev):
    run = ev["run"]
    return dict(updated=int(run.sum()), skipped_nan=int((~run).sum()), sigma2_restored=int(ev["restored"].sum()),
                mu_reset=int(ev["reset"].sum()), converged=int(ev["converged"].sum()))


def reproject_tracks(norm_xy, rho, K4, p, q):
    """Tracker::getCoord's track (Tracker.cpp:343-366) in fp64 from the fp32 planes, as the device's EDS_DEPTH_REPROJECT forms it"""
    fx, fy = K4[0], K4[1]
    x = np.asarray(norm_xy[:, 0], dtype=np.float32).astype(np.float64)
    y = np.asarray(norm_xy[:, 1], dtype=np.float32).astype(np.float64)
    r = np.asarray(rho, dtype=np.float32).astype(np.float64)
    D = quat_to_RmI(q)
    d0 = D[0, 0] * x + D[0, 1] * y + D[0, 2] + p[0] * r
    d1 = D[1, 0] * x + D[1, 1] * y + D[1, 2] + p[1] * r
    d2 = D[2, 0] * x + D[2, 1] * y + D[2, 2] + p[2] * r
    inv = 1.0 / (1.0 + d2)
    return np.stack([fx * (d0 - x * d2) * inv, fy * (d1 - y * d2) * inv], axis=1)


def slot_pixels(norm_xy, K4):
    """the keyframe pixel a tracker slot holds: u0 = fx x + cy in fp64, split into an integer cell and an fp32 fraction"""
    u0 = K4[0] * norm_xy[:, 0] + K4[2]
    v0 = K4[1] * norm_xy[:, 1] + K4[3]
    cu, cv = np.floor(u0), np.floor(v0)
    return np.stack([cu + (u0 - cu).astype(np.float32).astype(np.float64), cv + (v0 - cv).astype(np.float32).astype(np.float64)], axis=1)


def mean_std_vector(x):
    """Utils.hpp:272-290: (mean, VARIANCE with n-1), (x[0], 0) for n = 1; sequential sums like std::accumulate"""
    x = [float(v) for v in x]
    n = len(x)
    if n == 1:
        return x[0], 0.0
    acc = 0.0
    for v in x:
        acc += v
    mu = acc / n
    var = 0.0
    for v in x:
        var += (v - mu) * (v - mu) / (n - 1)
    return mu, var


def median_idepth(x):
    """medianIDepth (DepthPoints.cpp:255-260): nth_element at n/2 and, as "third_q", at n/3"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = len(x)
    return float(x[n // 2]), float(x[n // 3])
