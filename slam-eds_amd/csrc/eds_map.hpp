// The map as a point cloud and as the next keyframe's depth map (include/eds_hip_map.h): what the device kernels (eds_map.hip) and the
// host share — the back-projection of a window point with getMap's mixed widths, the fan of eight points, the immature points'
// depth and colour, the rigid transform in its one summation order, IDepthMap::fromPoints' projection and inlier rule — and the serial
// forms of the four clouds, which the tests and the timing's host leg run.  Written from the reference's lines (src/io/OutputMaps.cpp:38-148,
// src/tracking/KeyFrame.cpp:1244-1300, src/mapping/Types.hpp:248-275); every operation is one correctly rounded IEEE operation, no
// product is contracted into a sum (both sides are built with -ffp-contract=off), so host and device give the same bits.  Plain C++ outside
// hipcc.
#pragma once
#include <cmath>
#include <cstdint>

#include "eds_dso_common.hpp"

namespace edsmap {

constexpr int MAX_FRAMES = 8;                                   // hosts of a window (eds_hip_window.h)
constexpr int MAX_IMM_HOSTS = 32;                               // hosts of an immature cloud: one bit each of host_mask
constexpr int FAN = 8;                                          // points per map point when single_point == 0
constexpr int CHUNK = 1024;                                     // the compacting kernels' workgroup: points per sweep
constexpr int NUM_STATUS = 6;                                   // ImmaturePointStatus

struct Calib { float fx, fy, cx, cy; };                         // hcalib->fxl() .. cyl(), narrowed to float as getMap narrows them (:42-45)

// the hosts' runs of a window's point table: host h holds points first[h] .. first[h + 1] - 1
struct Runs { int32_t first[MAX_FRAMES + 1]; };

// getMap's eight points (:55-84): the centre, then (0,+2) (-1,+1) (-2,0) (-1,-1) (0,-2) (+1,-1) (+2,0)
EDS_HD int fan_dx(int k) { const int t[FAN] = {0, 0, -1, -2, -1, 0, 1, 2}; return t[k]; }
EDS_HD int fan_dy(int k) { const int t[FAN] = {0, 2, 1, 0, -1, -2, -1, 0}; return t[k]; }

// p->u - 1 - cx and its kin: fp32, left to right; an offset of 0 is not added (p->u - cx)
EDS_HD float fan_coord(float u, int d, float c) {
    float a = u;
    if (d != 0) a = a + (float)d;
    return a - c;
}

// ::base::Point(d_i * (p->u - cx) / fx, d_i * (p->v - cy) / fy, d_i) for point k of the fan: the difference in fp32, the product and the
// quotient in fp64, (d_i * a) / fx
EDS_HD void back_project(const Calib& c, float u, float v, double d_i, int k, double* P) {
    const float a = fan_coord(u, fan_dx(k), c.cx), b = fan_coord(v, fan_dy(k), c.cy);
    P[0] = (d_i * (double)a) / (double)c.fx;
    P[1] = (d_i * (double)b) / (double)c.fy;
    P[2] = d_i;
}

// T * p, T the rows of [R | t]: R_i0 X + R_i1 Y + R_i2 Z + t_i summed left to right (the order include/eds_hip_kfpoints.h states)
EDS_HD void transform(const double* T, const double* p, double* o) {
    for (int i = 0; i < 3; ++i) o[i] = T[4 * i] * p[0] + T[4 * i + 1] * p[1] + T[4 * i + 2] * p[2] + T[4 * i + 3];
}

// getMap: d_i = 1.0 / p->idepth_scaled (:51); no test, a zero, negative or NaN inverse depth gives the point it gives
EDS_HD double window_depth(float idepth_scaled) { return 1.0 / (double)idepth_scaled; }

// getImmatureMap: d_i = 1.0 / (0.5 * (idepth_max + idepth_min)) (:107), the sum in fp32; false where the reference skips the point
// (:109), and for a point that is not alive: it is no longer in immaturePoints
EDS_HD bool immature_depth(int32_t alive, float idepth_min, float idepth_max, double* d_i) {
    const float s = idepth_max + idepth_min;
    const double d = 1.0 / (0.5 * (double)s);
    *d_i = d;
    if (!alive) return false;
    if (d < 0) return false;
    return fabs(d) <= 1.7976931348623157e308;                  // std::isfinite: false for NaN and +-inf
}

// getImmatureMap's colour by lastTraceStatus (:112-123): GOOD green, OOB red, OUTLIER blue, SKIPPED cyan, BADCONDITION white,
// UNINITIALIZED black.  A code outside the table leaves the reference's colour uninitialised; here it is four zeros.
EDS_HD void status_color(int32_t status, double* c) {
    const double t[NUM_STATUS][4] = {{0, 1, 0, 1}, {1, 0, 0, 1}, {0, 0, 1, 1}, {0, 1, 1, 1}, {1, 1, 1, 1}, {0, 0, 0, 1}};
    for (int i = 0; i < 4; ++i) c[i] = status >= 0 && status < NUM_STATUS ? t[status][i] : 0.0;
}

// IDepthMap::fromPoints (Types.hpp:264-267): px = fx (X / Z) + cx, py likewise, idp = 1 / Z; kept iff 0 <= px < W and 0 <= py < H,
// written so that a NaN fails.  K: fx, fy, cx, cy.  Z <= 0 is not tested, as there.
EDS_HD bool project(const double* K, double W, double H, const double* P, double* px, double* py, double* idp) {
    *px = K[0] * (P[0] / P[2]) + K[2];
    *py = K[1] * (P[1] / P[2]) + K[3];
    *idp = 1.0 / P[2];
    return *px >= 0.0 && *px < W && *py >= 0.0 && *py < H;
}

// point k of window point (u, v, idepth_scaled) of a host with pose T_w_c, in the world
EDS_HD void window_point(const Calib& c, const double* T_w_c, float u, float v, float idepth_scaled, int k, double* o) {
    double P[3];
    back_project(c, u, v, window_depth(idepth_scaled), k, P);
    transform(T_w_c, P, o);
}

// KeyFrame::getMap (:1260-1262): T_w_kf * (d x_n, d y_n, d), d = 1.0 / idp
EDS_HD void slot_point(const double* T_w_kf, double xn, double yn, double idp, double* o) {
    const double d = 1.0 / idp;
    const double P[3] = {d * xn, d * yn, d};
    transform(T_w_kf, P, o);
}

inline bool finite_all(const double* p, int64_t n) {
    for (int64_t i = 0; i < n; ++i) if (!edsdso::finite_d(p[i])) return false;
    return true;
}

// the runs of a point table whose hosts do not decrease; false where they do, or where a host is outside 0 .. F - 1
inline bool make_runs(int n, const int32_t* host, int F, Runs* r) {
    for (int p = 0; p < n; ++p)
        if (host[p] < 0 || host[p] >= F || (p && host[p] < host[p - 1])) return false;
    for (int f = 0, p = 0; f <= MAX_FRAMES; ++f) {
        r->first[f] = p;
        while (p < n && host[p] == f) ++p;
    }
    return true;
}
// points of the hosts whose bit is set in mask (bits at and above F are ignored); per_host (may be NULL): [8], 0 for the others
inline int selected_points(const Runs& r, int F, uint32_t mask, int32_t* per_host) {
    int total = 0;
    for (int f = 0; f < MAX_FRAMES; ++f) {
        const int c = f < F && ((mask >> f) & 1u) ? r.first[f + 1] - r.first[f] : 0;
        if (per_host) per_host[f] = c;
        total += c;
    }
    return total;
}

// ---- the serial forms ------------------------------------------------------------------------------------------------------------------
// dso::io::getMap for every selected host, hosts in window order, each host's points in table order; uv: n x 2; T_w_c: F x 12;
// points: the count returned x 3
inline int64_t window_cloud(const Runs& r, const float* uv, const float* ids, const Calib& c, int F, uint32_t mask, const double* T_w_c,
                            int single_point, double* points) {
    int64_t q = 0;
    const int fan = single_point ? 1 : FAN;
    for (int h = 0; h < F; ++h) {
        if (!((mask >> h) & 1u)) continue;
        for (int p = r.first[h]; p < r.first[h + 1]; ++p)
            for (int k = 0; k < fan; ++k, ++q) window_point(c, T_w_c + 12 * h, uv[2 * p], uv[2 * p + 1], ids[p], k, points + 3 * q);
    }
    return q;
}

// the single-point cloud, each world point moved by T_dst_w[b] and pushed through fromPoints with K_dst[b] and {dst_W, dst_H}; map b
// starts at point b * stride; src (may be NULL): the table index of every kept point
inline void window_depth_maps(const Runs& r, const float* uv, const float* ids, const Calib& c, int F, uint32_t mask, const double* T_w_c,
                              int count, const double* T_dst_w, const double* K_dst, int dst_H, int dst_W, int64_t stride, double* xy,
                              double* idp, int32_t* src, int32_t* n_out) {
    for (int b = 0; b < count; ++b) {
        int64_t q = (int64_t)b * stride;
        for (int h = 0; h < F; ++h) {
            if (!((mask >> h) & 1u)) continue;
            for (int p = r.first[h]; p < r.first[h + 1]; ++p) {
                double w[3], d[3], px, py, ip;
                window_point(c, T_w_c + 12 * h, uv[2 * p], uv[2 * p + 1], ids[p], 0, w);
                transform(T_dst_w + 12 * b, w, d);
                if (!project(K_dst + 4 * b, (double)dst_W, (double)dst_H, d, &px, &py, &ip)) continue;
                xy[2 * q] = px; xy[2 * q + 1] = py; idp[q] = ip;
                if (src) src[q] = p;
                ++q;
            }
        }
        n_out[b] = (int32_t)(q - (int64_t)b * stride);
    }
}

// getImmatureMap for every selected host; host h's points are first[h] .. first[h + 1] - 1 of the arrays; colors (x 4) and status_out
// may be NULL.  With points == NULL nothing is written: the count alone.
inline int64_t immature_cloud(int n_hosts, uint32_t mask, const int32_t* first, const float* uv, const float* idepth_min, const float* idepth_max,
                              const int32_t* status, const int32_t* alive, const double* T_w_c, const Calib& c, int single_point, double* points,
                              double* colors, uint8_t* status_out) {
    int64_t q = 0;
    const int fan = single_point ? 1 : FAN;
    for (int h = 0; h < n_hosts; ++h) {
        if (!((mask >> h) & 1u)) continue;
        for (int p = first[h]; p < first[h + 1]; ++p) {
            double d_i;
            if (!immature_depth(alive[p], idepth_min[p], idepth_max[p], &d_i)) continue;
            for (int k = 0; k < fan; ++k, ++q) {
                if (!points) continue;
                double P[3];
                back_project(c, uv[2 * p], uv[2 * p + 1], d_i, k, P);
                transform(T_w_c + 12 * h, P, points + 3 * q);
                if (colors) status_color(status[p], colors + 4 * q);
                if (status_out) status_out[q] = (uint8_t)status[p];
            }
        }
    }
    return q;
}

// KeyFrame::getMap's points of one slot: n points, xn / yn the stored fp32 normalised coordinates, idp the inverse depths as fp64
inline void slot_cloud(int n, const float* xn, const float* yn, const double* idp, const double* T_w_kf, double* points) {
    for (int i = 0; i < n; ++i) slot_point(T_w_kf, (double)xn[i], (double)yn[i], idp[i], points + 3 * i);
}

}  // namespace edsmap
