// include/eds_hip_undistort.h: what the kernels of eds_undistort.hip and the host share.  Two halves:
//  - the SET-UP, host code only (it calls the C library's tanf, atanf, atan2f, sqrtf, whose bits a device math library does not give):
//    readFromFile from the point where the numbers are known, makeOptimalK_crop, the five distortCoordinates, the "rounding resistant"
//    pass, and PhotometricUndistorter's constructor after its file reads.  eds_und_create and eds_und_set_photometric run it inside the
//    library; tests/host_logic/undistort_harness.cpp compiles the very same text with g++.
//  - the PER-PIXEL arithmetic of processFrame<T> and of undistort<T>'s bilinear remap, __host__ __device__: corrected() and bilinear().
//    The kernels call them per tap; process_host() below is the reference's two passes over them, for the tests and for scale.
// Everything is written in the reference's types and order (reference src/utils/Undistort.cpp, line numbers below); build without
// contraction into FMAs.  The kept quirks and the defined rules are listed in the header.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "eds_dso_common.hpp"

namespace edsund {

constexpr int MIN_SIDE = 8, MAX_SIDE = 8192, MAX_SLOTS = 16;
constexpr int CROP_ITERATIONS = 500;          // :688
constexpr int LINE_SAMPLES = 100000;          // :586
constexpr int MIN_G_DEPTH = 256, MAX_G_DEPTH = 256 * 256;
enum { MODEL_FOV = 0, MODEL_RADTAN = 1, MODEL_EQUIDISTANT = 2, MODEL_KB = 3, MODEL_PINHOLE = 4 };
enum { OUT_CROP = 0, OUT_NONE = 1, OUT_GIVEN = 2, OUT_FULL = 3 };
enum { RAW_U8 = 0, RAW_U16 = 1 };
enum { RC_OK = 0, RC_INVALID = -1, RC_NOT_USABLE = -3 };       // the values of eds_status

struct Geometry {           // eds_und_geometry member for member
    int32_t model;
    double pars[8];
    int32_t w_org, h_org;
    int32_t out_mode;
    float out_pars[5];
    int32_t w, h;
};

struct Settings {           // eds_und_settings member for member
    int32_t photometric_calibration;
    int32_t use_exposure;
};
inline Settings settings_default() { return Settings{2, 1}; }      // settings.cpp:117-118
inline bool settings_valid(const Settings& s) {
    return s.photometric_calibration >= 0 && s.photometric_calibration <= 2 && (s.use_exposure == 0 || s.use_exposure == 1);
}

// ---- per pixel, host and device ------------------------------------------------------------------------------------------------

// processFrame<T> (:214-234) for one pixel: `phot` is valid && exposure > 0 && setting_photometricCalibration != 0, `vig` is
// setting_photometricCalibration == 2.  One fp32 product of two table reads, so a tap corrected on the fly has the plane's bits.
EDS_HD float corrected(int raw, bool phot, bool vig, const float* G, const float* vinv, int64_t i, float factor) {
    if (!phot) return factor * (float)raw;
    float v = G[raw];
    if (vig) v = v * vinv[i];
    return v;
}
// processFrame's branch for one frame; NaN is not <= 0
EDS_HD bool photometric_branch(bool valid, float exposure, int mode) { return !(!valid || exposure <= 0 || mode == 0); }

// :437: the reference tests xx < 0; a NaN, which no checked map holds, counts as outside here
EDS_HD bool outside(float xx) { return !(xx >= 0.0f); }

// :452-455 from the four taps: src[0], src[1], src[wOrg], src[1 + wOrg] and the fractions; every sum left to right
EDS_HD float bilinear(float xx, float yy, float s0, float s1, float sw, float sw1) {
    const float xxyy = xx * yy;
    return ((xxyy * sw1 + (yy - xxyy) * sw) + (xx - xxyy) * s1) + (((1.0f - xx) - yy) + xxyy) * s0;
}

// a map pair eds_und_set_map accepts, and the only kind the set-up produces: (-1, -1) or strictly inside the raw image, so that the
// four taps of (int)x, (int)y exist
inline bool map_pair_valid(float x, float y, int w_org, int h_org) {
    if (x == -1.0f && y == -1.0f) return true;
    return std::isfinite(x) && std::isfinite(y) && x > 0.0f && y > 0.0f && x < (float)(w_org - 1) && y < (float)(h_org - 1);
}

// ---- set-up: host only ---------------------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)

// the five distortCoordinates (:961-1225); in and out may be the same arrays, as the reference calls them
inline void distort(int model, const double* parsOrg, const double* K, const float* in_x, const float* in_y, float* out_x, float* out_y, int n) {
    const float fx = (float)parsOrg[0], fy = (float)parsOrg[1], cx = (float)parsOrg[2], cy = (float)parsOrg[3];
    const float ofx = (float)K[0], ofy = (float)K[4], ocx = (float)K[2], ocy = (float)K[5];
    if (model == MODEL_FOV) {
        const float dist = (float)parsOrg[4];
        const float d2t = 2.0f * tanf(dist / 2.0f);
        for (int i = 0; i < n; i++) {
            const float x = in_x[i], y = in_y[i];
            float ix = (x - ocx) / ofx;
            float iy = (y - ocy) / ofy;
            const float r = sqrtf(ix * ix + iy * iy);
            const float fac = (r == 0 || dist == 0) ? 1.0f : atanf(r * d2t) / (dist * r);
            ix = fx * fac * ix + cx;
            iy = fy * fac * iy + cy;
            out_x[i] = ix;
            out_y[i] = iy;
        }
    } else if (model == MODEL_RADTAN) {
        const float k1 = (float)parsOrg[4], k2 = (float)parsOrg[5], r1 = (float)parsOrg[6], r2 = (float)parsOrg[7];
        for (int i = 0; i < n; i++) {
            const float x = in_x[i], y = in_y[i];
            const float ix = (x - ocx) / ofx;
            const float iy = (y - ocy) / ofy;
            const float mx2_u = ix * ix;
            const float my2_u = iy * iy;
            const float mxy_u = ix * iy;
            const float rho2_u = mx2_u + my2_u;
            const float rad_dist_u = k1 * rho2_u + k2 * rho2_u * rho2_u;
            // float + double + double: the 2.0 makes the last two terms products and sums of doubles
            const float x_dist = (float)(((double)(ix + ix * rad_dist_u) + 2.0 * (double)r1 * (double)mxy_u) + (double)r2 * ((double)rho2_u + 2.0 * (double)mx2_u));
            const float y_dist = (float)(((double)(iy + iy * rad_dist_u) + 2.0 * (double)r2 * (double)mxy_u) + (double)r1 * ((double)rho2_u + 2.0 * (double)my2_u));
            out_x[i] = fx * x_dist + cx;
            out_y[i] = fy * y_dist + cy;
        }
    } else if (model == MODEL_EQUIDISTANT) {
        const float k1 = (float)parsOrg[4], k2 = (float)parsOrg[5], k3 = (float)parsOrg[6], k4 = (float)parsOrg[7];
        for (int i = 0; i < n; i++) {
            const float x = in_x[i], y = in_y[i];
            const float ix = (x - ocx) / ofx;
            const float iy = (y - ocy) / ofy;
            const float r = sqrtf(ix * ix + iy * iy);
            const float theta = atanf(r);
            const float theta2 = theta * theta;
            const float theta4 = theta2 * theta2;
            const float theta6 = theta4 * theta2;
            const float theta8 = theta4 * theta4;
            const float thetad = theta * (1.0f + k1 * theta2 + k2 * theta4 + k3 * theta6 + k4 * theta8);
            const float scaling = ((double)r > 1e-8) ? thetad / r : 1.0f;
            out_x[i] = fx * ix * scaling + cx;
            out_y[i] = fy * iy * scaling + cy;
        }
    } else if (model == MODEL_KB) {
        const float k0 = (float)parsOrg[4], k1 = (float)parsOrg[5], k2 = (float)parsOrg[6], k3 = (float)parsOrg[7];
        for (int i = 0; i < n; i++) {
            const float x = in_x[i], y = in_y[i];
            const float ix = (x - ocx) / ofx;
            const float iy = (y - ocy) / ofy;
            const float Xsq_plus_Ysq = ix * ix + iy * iy;
            const float sqrt_Xsq_Ysq = sqrtf(Xsq_plus_Ysq);
            const float theta = atan2f(sqrt_Xsq_Ysq, 1.0f);
            const float theta2 = theta * theta;
            const float theta3 = theta2 * theta;
            const float theta5 = theta3 * theta2;
            const float theta7 = theta5 * theta2;
            const float theta9 = theta7 * theta2;
            const float r = theta + k0 * theta3 + k1 * theta5 + k2 * theta7 + k3 * theta9;
            if ((double)sqrt_Xsq_Ysq < 1e-6) {
                out_x[i] = fx * ix + cx;
                out_y[i] = fy * iy + cy;
            } else {
                out_x[i] = (r / sqrt_Xsq_Ysq) * fx * ix + cx;
                out_y[i] = (r / sqrt_Xsq_Ysq) * fy * iy + cy;
            }
        }
    } else {        // MODEL_PINHOLE
        for (int i = 0; i < n; i++) {
            const float x = in_x[i], y = in_y[i];
            float ix = (x - ocx) / ofx;
            float iy = (y - ocy) / ofy;
            ix = fx * ix + cx;
            iy = fy * iy + cy;
            out_x[i] = ix;
            out_y[i] = iy;
        }
    }
}

struct __attribute__((visibility("default"))) Setup {          // a type, unlike the functions around it, may be named by a caller's own types
    Geometry g;                     // pars after the relative-format rescale
    double K[9];
    bool passthrough = false;
    bool relative = false;          // the rescale ran
    int iterations = 0;             // of the crop loop
    int shrinks[4] = {0, 0, 0, 0};  // how often it shrank left, right, top, bottom
    float range[4] = {0, 0, 0, 0};  // minX, maxX, minY, maxY before the loop, after the 1.01 widening
    int64_t rule_pixels = 0;        // map pixels defined rule (1) turned into (-1, -1)
    std::vector<float> mapx, mapy;  // remapX, remapY
};

inline void set_identity(double* K) {
    for (int i = 0; i < 9; ++i) K[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

// makeOptimalK_crop (:580-700); remapX / remapY are the w * h scratch the reference uses (w * h >= 2 * max(w, h) from MIN_SIDE on)
inline int optimal_K_crop(Setup& s) {
    const Geometry& g = s.g;
    const int w = g.w, h = g.h, wOrg = g.w_org, hOrg = g.h_org;
    double* K = s.K;
    float* remapX = s.mapx.data();
    float* remapY = s.mapy.data();
    set_identity(K);

    // 1. stretch the center lines as far as possible, to get initial coarse quess.
    std::vector<float> tgXv(LINE_SAMPLES), tgYv(LINE_SAMPLES);
    float* tgX = tgXv.data();
    float* tgY = tgYv.data();
    float minX = 0, maxX = 0, minY = 0, maxY = 0;
    for (int x = 0; x < LINE_SAMPLES; x++) { tgX[x] = (x - 50000.0f) / 10000.0f; tgY[x] = 0; }
    distort(g.model, g.pars, K, tgX, tgY, tgX, tgY, LINE_SAMPLES);
    for (int x = 0; x < LINE_SAMPLES; x++) {
        if (tgX[x] > 0 && tgX[x] < wOrg - 1) {
            if (minX == 0) minX = (x - 50000.0f) / 10000.0f;
            maxX = (x - 50000.0f) / 10000.0f;
        }
    }
    for (int y = 0; y < LINE_SAMPLES; y++) { tgY[y] = (y - 50000.0f) / 10000.0f; tgX[y] = 0; }
    distort(g.model, g.pars, K, tgX, tgY, tgX, tgY, LINE_SAMPLES);
    for (int y = 0; y < LINE_SAMPLES; y++) {
        if (tgY[y] > 0 && tgY[y] < hOrg - 1) {
            if (minY == 0) minY = (y - 50000.0f) / 10000.0f;
            maxY = (y - 50000.0f) / 10000.0f;
        }
    }
    minX = (float)(minX * 1.01);
    maxX = (float)(maxX * 1.01);
    minY = (float)(minY * 1.01);
    maxY = (float)(maxY * 1.01);
    s.range[0] = minX; s.range[1] = maxX; s.range[2] = minY; s.range[3] = maxY;

    // 2. while there are invalid pixels at the border: shrink square at the side that has invalid pixels,
    // if several to choose from, shrink the wider dimension.
    bool oobLeft = true, oobRight = true, oobTop = true, oobBottom = true;
    int iteration = 0;
    while (oobLeft || oobRight || oobTop || oobBottom) {
        oobLeft = oobRight = oobTop = oobBottom = false;
        for (int y = 0; y < h; y++) {
            remapX[y * 2] = minX;
            remapX[y * 2 + 1] = maxX;
            remapY[y * 2] = remapY[y * 2 + 1] = minY + (maxY - minY) * (float)y / ((float)h - 1.0f);
        }
        distort(g.model, g.pars, K, remapX, remapY, remapX, remapY, 2 * h);
        for (int y = 0; y < h; y++) {
            if (!(remapX[2 * y] > 0 && remapX[2 * y] < wOrg - 1)) oobLeft = true;
            if (!(remapX[2 * y + 1] > 0 && remapX[2 * y + 1] < wOrg - 1)) oobRight = true;
        }
        for (int x = 0; x < w; x++) {
            remapY[x * 2] = minY;
            remapY[x * 2 + 1] = maxY;
            remapX[x * 2] = remapX[x * 2 + 1] = minX + (maxX - minX) * (float)x / ((float)w - 1.0f);
        }
        distort(g.model, g.pars, K, remapX, remapY, remapX, remapY, 2 * w);
        for (int x = 0; x < w; x++) {
            if (!(remapY[2 * x] > 0 && remapY[2 * x] < hOrg - 1)) oobTop = true;
            if (!(remapY[2 * x + 1] > 0 && remapY[2 * x + 1] < hOrg - 1)) oobBottom = true;
        }
        if ((oobLeft || oobRight) && (oobTop || oobBottom)) {
            if ((maxX - minX) > (maxY - minY))
                oobBottom = oobTop = false;     // only shrink left/right
            else
                oobLeft = oobRight = false;     // only shrink top/bottom
        }
        if (oobLeft) { minX = (float)(minX * 0.995); s.shrinks[0]++; }
        if (oobRight) { maxX = (float)(maxX * 0.995); s.shrinks[1]++; }
        if (oobTop) { minY = (float)(minY * 0.995); s.shrinks[2]++; }
        if (oobBottom) { maxY = (float)(maxY * 0.995); s.shrinks[3]++; }
        iteration++;
        s.iterations = iteration;
        if (iteration > CROP_ITERATIONS) return RC_NOT_USABLE;      // the reference: exit(1)
    }
    K[0] = ((float)w - 1.0f) / (maxX - minX);
    K[4] = ((float)h - 1.0f) / (maxY - minY);
    K[2] = -minX * K[0];
    K[5] = -minY * K[4];
    return RC_OK;
}

inline bool geometry_valid(const Geometry& g) {
    if (g.model < MODEL_FOV || g.model > MODEL_PINHOLE) return false;
    if (g.out_mode != OUT_CROP && g.out_mode != OUT_NONE && g.out_mode != OUT_GIVEN) return false;      // "full": the reference asserts
    for (int v : {g.w_org, g.h_org, g.w, g.h})
        if (v < MIN_SIDE || v > MAX_SIDE) return false;
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(g.pars[i])) return false;
    if (g.out_mode == OUT_GIVEN)
        for (int i = 0; i < 5; ++i)
            if (!std::isfinite(g.out_pars[i])) return false;
    if (g.out_mode == OUT_NONE && (g.w != g.w_org || g.h != g.h_org)) return false;
    return true;
}

// readFromFile from :782 on.  RC_INVALID (nothing of `s` is meaningful), RC_NOT_USABLE (the crop loop ran out), RC_OK.
inline int setup(const Geometry& geometry, Setup& s) {
    if (!geometry_valid(geometry)) return RC_INVALID;
    s = Setup();
    s.g = geometry;
    Geometry& g = s.g;
    double* parsOrg = g.pars;
    const int w = g.w, h = g.h, wOrg = g.w_org, hOrg = g.h_org;
    if (parsOrg[2] < 1 && parsOrg[3] < 1) {
        // rescale and substract 0.5 offset.
        parsOrg[0] = parsOrg[0] * wOrg;
        parsOrg[1] = parsOrg[1] * hOrg;
        parsOrg[2] = parsOrg[2] * wOrg - 0.5;
        parsOrg[3] = parsOrg[3] * hOrg - 0.5;
        s.relative = true;
    }
    s.mapx.assign((size_t)w * h, 0.0f);
    s.mapy.assign((size_t)w * h, 0.0f);
    float* remapX = s.mapx.data();
    float* remapY = s.mapy.data();
    double* K = s.K;
    if (g.out_mode == OUT_CROP) {
        if (int rc = optimal_K_crop(s)) return rc;
    } else if (g.out_mode == OUT_NONE) {
        set_identity(K);
        K[0] = parsOrg[0];
        K[4] = parsOrg[1];
        K[2] = parsOrg[2];
        K[5] = parsOrg[3];
        s.passthrough = true;
    } else {
        const float* outputCalibration = g.out_pars;
        set_identity(K);
        K[0] = outputCalibration[0] * w;
        K[4] = outputCalibration[1] * h;
        K[2] = outputCalibration[2] * w - 0.5;
        K[5] = outputCalibration[3] * h - 0.5;
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            remapX[x + y * w] = x;
            remapY[x + y * w] = y;
        }
    distort(g.model, parsOrg, K, remapX, remapY, remapX, remapY, h * w);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            // make rounding resistant.
            float ix = remapX[x + y * w];
            float iy = remapY[x + y * w];
            if (ix == 0) ix = 0.001;
            if (iy == 0) iy = 0.001;
            if (ix == wOrg - 1) ix = wOrg - 1.001;
            if (iy == hOrg - 1) ix = hOrg - 1.001;      // kept: ix
            const bool reference_test = ix > 0 && iy > 0 && ix < wOrg - 1 && iy < wOrg - 1;     // kept: wOrg
            const bool rows_exist = iy < hOrg - 1;                                                // defined rule (1)
            if (reference_test && !rows_exist) s.rule_pixels++;
            if (reference_test && rows_exist) {
                remapX[x + y * w] = ix;
                remapY[x + y * w] = iy;
            } else {
                remapX[x + y * w] = -1;
                remapY[x + y * w] = -1;
            }
        }
    return RC_OK;
}

inline bool map_valid(const float* mapx, const float* mapy, size_t n, int w_org, int h_org) {
    for (size_t i = 0; i < n; ++i)
        if (!map_pair_valid(mapx[i], mapy[i], w_org, h_org)) return false;
    return true;
}

// PhotometricUndistorter's constructor after its file reads (:79-170)
struct __attribute__((visibility("default"))) Photometric {
    bool valid = false;
    int g_depth = 0;
    std::vector<float> G_given;         // rescaled to 0 .. 255 (:101)
    std::vector<float> G;               // what processFrame reads: G_given, or the line of :106 in mode 0
    std::vector<float> vignetteMapInv;
};

inline void apply_mode_to_G(Photometric& p, int mode) {
    if (!p.valid) return;
    p.G = p.G_given;
    if (mode == 0)
        for (int i = 0; i < p.g_depth; i++) p.G[i] = 255.0f * i / (float)(p.g_depth - 1);
}

// RC_INVALID leaves `p` as it was.  vignette: n = w_org * h_org values of uint8 (RAW_U8) or uint16 (RAW_U16).
inline int set_photometric(Photometric& p, const float* Gin, int g_depth, const void* vignette, int vignette_type, size_t n, int mode) {
    if (!Gin || !vignette || g_depth < MIN_G_DEPTH || g_depth > MAX_G_DEPTH) return RC_INVALID;
    if (vignette_type != RAW_U8 && vignette_type != RAW_U16) return RC_INVALID;
    for (int i = 0; i < g_depth - 1; i++)
        if (!(Gin[i + 1] > Gin[i])) return RC_INVALID;         // "has to be strictly increasing" (:92); a NaN is not
    std::vector<float> G(Gin, Gin + g_depth);
    const float min = G[0];
    const float max = G[g_depth - 1];
    for (int i = 0; i < g_depth; i++) G[i] = 255.0 * (G[i] - min) / (max - min);       // make it to 0..255 => 0..255.
    std::vector<float> vignetteMap(n), inv(n);
    float maxV = 0;
    if (vignette_type == RAW_U16) {
        const uint16_t* v = static_cast<const uint16_t*>(vignette);
        for (size_t i = 0; i < n; i++)
            if (v[i] > maxV) maxV = v[i];
        for (size_t i = 0; i < n; i++) vignetteMap[i] = v[i] / maxV;
    } else {
        const uint8_t* v = static_cast<const uint8_t*>(vignette);
        for (size_t i = 0; i < n; i++)
            if (v[i] > maxV) maxV = v[i];
        for (size_t i = 0; i < n; i++) vignetteMap[i] = v[i] / maxV;
    }
    for (size_t i = 0; i < n; i++) inv[i] = 1.0f / vignetteMap[i];
    p.valid = true;
    p.g_depth = g_depth;
    p.G_given.swap(G);
    p.vignetteMapInv.swap(inv);
    apply_mode_to_G(p, mode);
    return RC_OK;
}

// uint16 frames index G with up to 65 535
inline bool raw_type_fits(const Photometric& p, int mode, int raw_type) {
    return !(raw_type == RAW_U16 && p.valid && mode != 0 && p.g_depth < MAX_G_DEPTH);
}

// undistort<T> (:378-474) for one frame as the reference runs it: the photometric plane, then the remap (or the copy).
// `plane` is w_org * h_org floats of scratch, out is w * h.  Returns the frame's exposure_time.
template <class T>
inline float process_host(const Setup& s, const Photometric& p, const Settings& st, const T* raw, int64_t row_stride, float exposure, float factor,
                          float* plane, float* out) {
    const int wOrg = s.g.w_org, hOrg = s.g.h_org, w = s.g.w, h = s.g.h;
    const bool phot = photometric_branch(p.valid, exposure, st.photometric_calibration);
    const bool vig = st.photometric_calibration == 2;
    const float* G = p.valid ? p.G.data() : nullptr;
    const float* vinv = p.valid ? p.vignetteMapInv.data() : nullptr;
    for (int y = 0; y < hOrg; ++y)
        for (int x = 0; x < wOrg; ++x) {
            const int64_t i = (int64_t)y * wOrg + x;
            plane[i] = corrected((int)raw[(int64_t)y * row_stride + x], phot, vig, G, vinv, i, factor);
        }
    if (!s.passthrough) {
        for (int idx = w * h - 1; idx >= 0; idx--) {
            float xx = s.mapx[idx];
            float yy = s.mapy[idx];
            if (outside(xx))
                out[idx] = 0;
            else {
                const int xxi = xx;
                const int yyi = yy;
                xx -= xxi;
                yy -= yyi;
                const float* src = plane + xxi + yyi * wOrg;
                out[idx] = bilinear(xx, yy, src[0], src[1], src[wOrg], src[1 + wOrg]);
            }
        }
    } else {
        for (int64_t i = 0; i < (int64_t)w * h; ++i) out[i] = plane[i];
    }
    return st.use_exposure ? exposure : 1.0f;
}

#pragma GCC visibility pop

}  // namespace edsund
