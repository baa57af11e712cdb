"""The map's clouds and depth maps in plain numpy, line by line from the reference: ``dso::io::getMap`` and ``getImmatureMap``
(src/io/OutputMaps.cpp:38-148), ``KeyFrame::getMap``'s points (src/tracking/KeyFrame.cpp:1244-1300) and ``IDepthMap::fromPoints``
(src/mapping/Types.hpp:248-275), with the widths the C++ gives every operation.  Independent of csrc/eds_map.hpp: the tests compare the
two bit for bit.  A transform is ``R_i0 X + R_i1 Y + R_i2 Z + t_i`` summed left to right in fp64, the order include/eds_hip_map.h states
(Eigen's own order inside ``Transform * Vector3d`` is not pinned)."""
import numpy as np

f32, f64 = np.float32, np.float64
# the eight points of getMap (:55-84): (du, dv), the centre first
FAN = ((0, 0), (0, 2), (-1, 1), (-2, 0), (-1, -1), (0, -2), (1, -1), (2, 0))
# getImmatureMap's colours by lastTraceStatus (:112-123)
COLORS = np.array([[0, 1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 1]], dtype=f64)


def _offset(u, d, c):
    """p->u - 1 - cx and its kin: float arithmetic, left to right; (p->u - cx) where the source writes no offset"""
    a = u if d == 0 else (u + f32(d)).astype(f32)
    return (a - f32(c)).astype(f32)


def transform(T, P):
    """T: 12 doubles, rows of [R | t]; P: n x 3"""
    T = np.asarray(T, f64).reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1] + T[i, 2] * P[:, 2] + T[i, 3] for i in range(3)], axis=1)


def camera_points(uv, d_i, calib, single_point):
    """::base::Point(d_i*(p->u-cx)/fx, d_i*(p->v-cy)/fy, d_i) for every point and every point of its fan: n x fan x 3"""
    fx, fy, cx, cy = (f32(v) for v in calib)
    u, v = uv[:, 0].astype(f32), uv[:, 1].astype(f32)
    out = []
    with np.errstate(all="ignore"):
        for du, dv in (FAN[:1] if single_point else FAN):
            a, b = _offset(u, du, cx), _offset(v, dv, cy)
            out.append(np.stack([(d_i * a.astype(f64)) / f64(fx), (d_i * b.astype(f64)) / f64(fy), d_i], axis=1))
    return np.stack(out, axis=1)


def _selected(host, F, mask):
    """indices of the points of the selected hosts, hosts in window order, table order inside a host"""
    host = np.asarray(host)
    return np.concatenate([np.flatnonzero(host == h) for h in range(F) if (mask >> h) & 1] + [np.zeros(0, np.int64)]).astype(np.int64)


def window_cloud(host, uv, ids, calib, T_w_c, mask, single_point):
    """getMap over the window: (points n x 3, per_host[8])"""
    F = len(T_w_c)
    per = np.array([int(np.sum(np.asarray(host) == h)) if h < F and (mask >> h) & 1 else 0 for h in range(8)], np.int32)
    sel = _selected(host, F, mask)
    with np.errstate(all="ignore"):
        d_i = 1.0 / np.asarray(ids, f32)[sel].astype(f64)
    P = camera_points(np.asarray(uv, f32).reshape(-1, 2)[sel], d_i, calib, single_point)
    out = np.zeros(P.shape)
    for h in range(F):
        m = np.asarray(host)[sel] == h
        if m.any():
            out[m] = transform(T_w_c[h], P[m].reshape(-1, 3)).reshape(-1, P.shape[1], 3)
    return out.reshape(-1, 3), per


def from_points(points, K, W, H):
    """IDepthMap::fromPoints: (xy, idp, kept indices)"""
    fx, fy, cx, cy = (f64(v) for v in K)
    with np.errstate(all="ignore"):
        px = fx * (points[:, 0] / points[:, 2]) + cx
        py = fy * (points[:, 1] / points[:, 2]) + cy
        idp = 1.0 / points[:, 2]
        inlier = ((px >= 0.0) & (px < W)) & ((py >= 0.0) & (py < H))
    k = np.flatnonzero(inlier)
    return np.stack([px[k], py[k]], axis=1), idp[k], k


def window_depth_maps(host, uv, ids, calib, T_w_c, mask, T_dst_w, K_dst, dst_H, dst_W):
    """per destination: dict(xy, idp, src) — src the table index of every kept point"""
    F = len(T_w_c)
    world, _ = window_cloud(host, uv, ids, calib, T_w_c, mask, True)
    sel = _selected(host, F, mask)
    out = []
    for b in range(len(T_dst_w)):
        xy, idp, k = from_points(transform(T_dst_w[b], world), K_dst[b], dst_W, dst_H)
        out.append(dict(xy=xy, idp=idp, src=sel[k].astype(np.int32)))
    return out


def immature_cloud(n_per_host, uv, idepth_min, idepth_max, status, alive, T_w_c, calib, mask, single_point):
    """getImmatureMap over the hosts (arrays concatenated host after host): dict(points, colors, status)"""
    first = np.concatenate([[0], np.cumsum(n_per_host)])
    pts, cols, sts = [np.zeros((0, 3))], [np.zeros((0, 4))], [np.zeros(0, np.uint8)]
    for h in range(len(T_w_c)):
        if not (mask >> h) & 1:
            continue
        s = slice(first[h], first[h + 1])
        with np.errstate(all="ignore"):
            mid = (np.asarray(idepth_max, f32)[s] + np.asarray(idepth_min, f32)[s]).astype(f32)
            d_i = 1.0 / (0.5 * mid.astype(f64))
        keep = np.flatnonzero(np.asarray(alive)[s].astype(bool) & ~(d_i < 0) & np.isfinite(d_i))
        P = camera_points(np.asarray(uv, f32).reshape(-1, 2)[s][keep], d_i[keep], calib, single_point)
        fan = P.shape[1]
        pts.append(transform(T_w_c[h], P.reshape(-1, 3)))
        st = np.asarray(status, np.int32)[s][keep]
        cols.append(np.repeat(COLORS[st], fan, axis=0))
        sts.append(np.repeat(st.astype(np.uint8), fan))
    return dict(points=np.concatenate(pts), colors=np.concatenate(cols), status=np.concatenate(sts))


def slot_cloud(xn, yn, idp, T_w_kf):
    """KeyFrame::getMap: T_w_kf * (d_i x_n, d_i y_n, d_i), d_i = 1.0 / idp"""
    with np.errstate(all="ignore"):
        d = 1.0 / np.asarray(idp, f64)
        P = np.stack([d * np.asarray(xn, f64), d * np.asarray(yn, f64), d], axis=1)
    return transform(T_w_kf, P)


def bits(a):
    """an array as integers: the comparison is bit for bit, NaNs included"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])
