// DSO's coarse image tracker (include/eds_hip_coarse.h): what the device kernels (eds_coarse.hip) and the host share — makeK, every
// level of makeImages, the pieces of makeCoarseDepthL0, the per-point term of calcRes, the Jacobian row and the 45 products of
// calcGSSSE, the small solve, SE3::exp and the whole of trackNewestCoarse as a template over an EVALUATOR that supplies the two
// reductions — and a serial evaluator (SerialEval, track_serial) that walks the device's sum order.  fp32 per point in the
// reference's order, fp64 sums (E, the two flow sums, each of the 45 products over the list entries of a level) in THE SUM ORDER stated at
// the top of eds_dso_common.hpp, which also holds the pixel type, makeImages' level and gradient, the interpolation weights and the fold
// inside 64 lanes on the device; every translation unit that includes this is built without contraction into FMAs.  Plain C++ outside
// hipcc.
//
// sincos_d / exp_d are plain fp64 arithmetic (+, -, *, /, floor, integer bit moves), so g++ and gfx950 give the same bits.  The loop
// does not bound their arguments (an increment's angle and a difference of affine a's are whatever the solve gives), so the bounds
// are stated over everything the functions accept: against libm, sin and cos are within SINCOS_MAX_ULP = 2 ulps over |x| <= 2^20
// (NaN beyond), exp within EXP_MAX_ULP = 1 ulp over |x| <= 708 (inf and 0 beyond).  Measured: sin 2, cos 2, exp 1;
// tests/test_coarse_header.py asserts these constants.  atan_d (the initialiser's SE3::log, eds_init.hpp) is of the same kind: |x| > 1
// goes through 1 / |x|, the argument is reduced by the nearest c = k / 8 to r = (|x| - c) / (1 + |x| c), |r| <= 1/16, Taylor to r^19
// and atan(k / 8) from a table; within ATAN_MAX_ULP = 2 ulps of libm over every argument (NaN stays NaN, +-inf gives +-pi/2).
// Measured: 2 (near x = 1.06); tests/test_init_header.py asserts the constant.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "eds_dso_common.hpp"

namespace edsct {

using edsdso::finite_d;
using edsdso::finite_f;
using edsdso::LANES;
using edsdso::nan_d;
using edsdso::nan_f;
using edsdso::Px;

constexpr int MAX_LEVELS = 5;
constexpr int MAX_DECISIONS = 512;             // 10 + 20 + 3 * 100 iterations and one repeated level at the most
constexpr int NUM_SUMS = 45;
constexpr int SINCOS_MAX_ULP = 2;
constexpr int EXP_MAX_ULP = 1;
constexpr int ATAN_MAX_ULP = 2;

// eds_ct_params, member for member
struct Params { float huber_th, coarse_cutoff_th, affine_opt_mode_a, affine_opt_mode_b; };

struct Level { int32_t w, h, off, pad; float fx, fy, cx, cy, fxi, fyi, cxi, cyi; };
struct Geo { int32_t levels, W, H, total; Level l[MAX_LEVELS]; };

struct alignas(16) Pc { float u, v, idepth, color; };           // one entry of a level's pc_* lists

// the two frames' photometric state: AffLight::fromToVecExposure's arguments that do not change during a track
struct Photo { float exposure_ref, exposure_new; double ref_a, ref_b; };

// eds_ct_track's result for one try
struct TrackOut {
    double T[12], aff[2], last_residuals[5], flow[3];
    int32_t ok, n_decisions, iters[MAX_LEVELS], accepts[MAX_LEVELS];
    float cutoff_repeat; int32_t pad;
    uint8_t decisions[MAX_DECISIONS];                           // accept (bit 0) and level (bits 1 ..) of every iteration, in order
};

// what calcRes decides for one list entry
struct Term {
    int32_t in_e, warped, flow;                                  // in_e without warped: a saturated term
    float e;                                                    // the entry's addend to E
    float idepth, u, v, dx, dy, residual, weight, ref_color;    // its buf_warped_* row when `warped`
    float t1, t2, rt1, rt2;                                     // the four flow addends when `flow`
};

EDS_HD Params params_default() { Params p = {9.0f, 20.0f, 1e12f, 1e8f}; return p; }
EDS_HD bool params_valid(const Params& p) {
    return finite_f(p.huber_th) && finite_f(p.coarse_cutoff_th) && finite_f(p.affine_opt_mode_a) && finite_f(p.affine_opt_mode_b) &&
           p.huber_th > 0.0f && p.coarse_cutoff_th > 0.0f;
}

// ---- fp64 sin, cos and exp in plain arithmetic -------------------------------------------------------------------------------------
// x = k pi/2 + r by a three-part pi/2 (k pio2_1 and k pio2_2 are exact for |k| < 2^20), Taylor to r^17 / r^16 on |r| <= pi/4.
EDS_HD void sincos_d(double x, double* s, double* c) {
    if (!(fabs(x) <= 1048576.0)) { *s = nan_d(); *c = nan_d(); return; }
    const double kf = floor(x * 6.36619772367581382433e-01 + 0.5);
    const double r = ((x - kf * 1.57079632673412561417e+00) - kf * 6.07710050630396597660e-11) - kf * 2.02226624879595063154e-21;
    const double z = r * r;
    double ps = -1.0 / 355687428096000.0;                                        // 17!
    ps = ps * z + 1.0 / 1307674368000.0;
    ps = ps * z - 1.0 / 6227020800.0;
    ps = ps * z + 1.0 / 39916800.0;
    ps = ps * z - 1.0 / 362880.0;
    ps = ps * z + 1.0 / 5040.0;
    ps = ps * z - 1.0 / 120.0;
    ps = ps * z + 1.0 / 6.0;
    const double sn = r - (r * z) * ps;
    double pc = 1.0 / 20922789888000.0;                                          // 16!
    pc = pc * z - 1.0 / 87178291200.0;
    pc = pc * z + 1.0 / 479001600.0;
    pc = pc * z - 1.0 / 3628800.0;
    pc = pc * z + 1.0 / 40320.0;
    pc = pc * z - 1.0 / 720.0;
    pc = pc * z + 1.0 / 24.0;
    const double cs = (1.0 - 0.5 * z) + (z * z) * pc;
    const int q = (int)((int64_t)kf & 3);
    *s = q == 0 ? sn : q == 1 ? cs : q == 2 ? -sn : -cs;
    *c = q == 0 ? cs : q == 1 ? -sn : q == 2 ? -cs : sn;
}

// x = k ln2 + r (k ln2_hi is exact), Taylor to r^13 on |r| <= ln2 / 2, times 2^k built from its bits.  Outside +-708: inf and 0.
EDS_HD double exp_d(double x) {
    if (!(x == x)) return x;
    if (x > 708.0) return 1.0 / 0.0;
    if (x < -708.0) return 0.0;
    const double kf = floor(x * 1.44269504088896338700e+00 + 0.5);
    const double r = (x - kf * 6.93147180369123816490e-01) - kf * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    const double e = (1.0 + r) + (r * r) * p;
    const uint64_t bits = (uint64_t)((int64_t)kf + 1023) << 52;
    double scale;
    memcpy(&scale, &bits, sizeof(scale));
    return e * scale;
}

// ---- fp64 atan in plain arithmetic ---------------------------------------------------------------------------------------------------
EDS_HD double atan_d(double x) {
    if (!(x == x)) return x;
    const double ATAN_K[9] = {0.0, 0.12435499454676144, 0.24497866312686414, 0.35877067027057225, 0.46364760900080609,
                              0.55859931534356244, 0.64350110879328437, 0.71882999962162453, 0.78539816339744828};
    double ax = fabs(x);
    const bool inv = ax > 1.0;
    if (inv) ax = 1.0 / ax;
    const double kf = floor(ax * 8.0 + 0.5), c = kf * 0.125;
    const double r = (ax - c) / (1.0 + ax * c), z = r * r;
    double p = 1.0 / 19.0;
    p = 1.0 / 17.0 - z * p;
    p = 1.0 / 15.0 - z * p;
    p = 1.0 / 13.0 - z * p;
    p = 1.0 / 11.0 - z * p;
    p = 1.0 / 9.0 - z * p;
    p = 1.0 / 7.0 - z * p;
    p = 1.0 / 5.0 - z * p;
    p = 1.0 / 3.0 - z * p;
    const int k = (int)kf;
    double base = 0.0;
EDS_UNROLL
    for (int q = 0; q < 9; ++q) if (q == k) base = ATAN_K[q];
    double a = base + (r - (r * z) * p);
    if (inv) a = (1.5707963267948966 - a) + 6.123233995736766e-17;
    return x < 0.0 ? -a : a;
}

// ---- makeK (CoarseTracker.cpp:93-122) -----------------------------------------------------------------------------------------------
EDS_HD bool shape_valid(int H, int W, int levels) {
    if (levels < 1 || levels > MAX_LEVELS || H < 8 || W < 8 || H > 8192 || W > 8192) return false;
    const int m = 1 << (levels - 1);
    return H % m == 0 && W % m == 0 && (H >> (levels - 1)) >= 8 && (W >> (levels - 1)) >= 8;
}

EDS_HD void make_shape(Geo& g, int H, int W, int levels) {
    g.levels = levels; g.W = W; g.H = H;
    int off = 0;
    for (int l = 0; l < MAX_LEVELS; ++l) {
        Level& L = g.l[l];
        L.w = l < levels ? W >> l : 0; L.h = l < levels ? H >> l : 0; L.off = off; L.pad = 0;
        L.fx = L.fy = L.cx = L.cy = L.fxi = L.fyi = L.cxi = L.cyi = 0.0f;
        off += L.w * L.h;
    }
    g.total = off;
}

// fx_l = fx_{l-1} * 0.5 and c_l = (c_0 + 0.5) / 2^l - 0.5 are formed in fp64 from the fp32 operands and narrowed on assignment, as the
// reference's float members make them; Ki is the closed form of the inverse of an upper-triangular K, in fp32.
EDS_HD void make_k(Geo& g, float fx, float fy, float cx, float cy) {
    g.l[0].fx = fx; g.l[0].fy = fy; g.l[0].cx = cx; g.l[0].cy = cy;
    for (int l = 1; l < g.levels; ++l) {
        g.l[l].fx = (float)(g.l[l - 1].fx * 0.5);
        g.l[l].fy = (float)(g.l[l - 1].fy * 0.5);
        g.l[l].cx = (float)((g.l[0].cx + 0.5) / (double)(1 << l) - 0.5);
        g.l[l].cy = (float)((g.l[0].cy + 0.5) / (double)(1 << l) - 0.5);
    }
    for (int l = 0; l < g.levels; ++l) {
        Level& L = g.l[l];
        L.fxi = 1.0f / L.fx; L.fyi = 1.0f / L.fy; L.cxi = -L.cx / L.fx; L.cyi = -L.cy / L.fy;
    }
}

// ---- makeCoarseDepthL0 (CoarseTracker.cpp:126-283) ----------------------------------------------------------------------------------
// u = (int)(x + 0.5f): truncation towards zero, so -1 < x + 0.5f < 0 is pixel 0.  false: the contribution is dropped.
EDS_HD bool splat_pixel(float x, float y, int W, int H, int* pix) {
    const float xf = x + 0.5f, yf = y + 0.5f;
    if (!(xf > -1.0f && xf < (float)W && yf > -1.0f && yf < (float)H)) return false;
    *pix = (int)xf + W * (int)yf;
    return true;
}
EDS_HD float splat_weight(float hdif) { return sqrtf((float)(1e-3 / (hdif + 1e-12))); }

EDS_HD float level_sum(const float* lm, int wlm1, int x, int y) {
    const int b = 2 * x + 2 * y * wlm1;
    return ((lm[b] + lm[b + 1]) + lm[b + wlm1]) + lm[b + wlm1 + 1];
}

// one pixel of the dilation, read from the undilated planes (the reference's _bak): diagonal neighbours at levels 0 and 1, the cross
// above.  A neighbour index outside 0 .. w h - 1 (the reference reads one element before and after the plane) counts as empty.
EDS_HD void dilate_at(const float* id_in, const float* ws_in, int w, int h, int lvl, int i, float* id_out, float* ws_out) {
    float id = id_in[i], ws = ws_in[i];
    if (i >= w && i < w * h - w && ws <= 0) {
        const int off[4] = {lvl < 2 ? 1 + w : 1, lvl < 2 ? -1 - w : -1, lvl < 2 ? w - 1 : w, lvl < 2 ? -w + 1 : -w};
        float sum = 0, num = 0, numn = 0;
        for (int k = 0; k < 4; ++k) {
            const int j = i + off[k];
            if (j >= 0 && j < w * h && ws_in[j] > 0) { sum += id_in[j]; num += ws_in[j]; numn++; }
        }
        if (numn > 0) { id = sum / numn; ws = num / numn; }
    }
    *id_out = id; *ws_out = ws;
}

// the normalisation of one pixel; true: the pixel enters the level's list
EDS_HD bool normalise_at(int x, int y, int w, int h, float color, float* id, float* ws) {
    if (x < 2 || x >= w - 2 || y < 2 || y >= h - 2) return false;
    if (*ws > 0) {
        *id = *id / *ws;
        if (!finite_f(color) || !(*id > 0)) { *id = -1.0f; return false; }      // the reference's `continue` leaves weightSums as it is
        *ws = 1.0f;
        return true;
    }
    *id = -1.0f; *ws = 1.0f;
    return false;
}

// ---- calcRes (CoarseTracker.cpp:349-498) --------------------------------------------------------------------------------------------
struct Warp {
    float RKi[9], t[3], aff0, aff1, b0;
    float fx, fy, cx, cy, fxi, fyi, cxi, cyi;
    float huber, cutoff, max_energy, wl3, hl3;
    int32_t w, h, lvl;
};

// AffLight::fromToVecExposure (NumType.h:175-187)
EDS_HD void from_to_exposure(const Photo& ph, double a_new, double b_new, double* a, double* b) {
    float ef = ph.exposure_ref, et = ph.exposure_new;
    if (ef == 0 || et == 0) { et = 1; ef = 1; }
    *a = exp_d(a_new - ph.ref_a) * et / ef;
    *b = b_new - *a * ph.ref_b;
}

EDS_HD Warp make_warp(const Level& L, int lvl, const Params& s, const Photo& ph, const double* R, const double* t, double a, double b,
                         float cutoff) {
    Warp w;
    float r[9];
    for (int i = 0; i < 9; ++i) r[i] = (float)R[i];
    // R.cast<float>() * Ki: every coefficient is ((r0 k0 + r1 k1) + r2 k2) over Ki's column, its zeros included
    for (int i = 0; i < 3; ++i) {
        w.RKi[3 * i + 0] = (r[3 * i] * L.fxi + r[3 * i + 1] * 0.0f) + r[3 * i + 2] * 0.0f;
        w.RKi[3 * i + 1] = (r[3 * i] * 0.0f + r[3 * i + 1] * L.fyi) + r[3 * i + 2] * 0.0f;
        w.RKi[3 * i + 2] = (r[3 * i] * L.cxi + r[3 * i + 1] * L.cyi) + r[3 * i + 2] * 1.0f;
    }
    for (int i = 0; i < 3; ++i) w.t[i] = (float)t[i];
    double aa, bb;
    from_to_exposure(ph, a, b, &aa, &bb);
    w.aff0 = (float)aa; w.aff1 = (float)bb; w.b0 = (float)ph.ref_b;
    w.fx = L.fx; w.fy = L.fy; w.cx = L.cx; w.cy = L.cy; w.fxi = L.fxi; w.fyi = L.fyi; w.cxi = L.cxi; w.cyi = L.cyi;
    w.huber = s.huber_th; w.cutoff = cutoff;
    w.max_energy = 2 * s.huber_th * cutoff - s.huber_th * s.huber_th;
    w.w = L.w; w.h = L.h; w.lvl = lvl;
    w.wl3 = (float)(L.w - 3); w.hl3 = (float)(L.h - 3);
    return w;
}

EDS_HD float shift_sq(float ku, float kv, float x, float y) { return (ku - x) * (ku - x) + (kv - y) * (kv - y); }

// one list entry i of the level whose new-frame pixels are `img`
EDS_HD Term point_term(const Warp& w, const Px* img, const Pc& p, int i) {
    Term o;
    o.in_e = 0; o.warped = 0; o.flow = 0; o.e = 0.0f;
    o.idepth = o.u = o.v = o.dx = o.dy = o.residual = o.weight = o.ref_color = 0.0f;
    o.t1 = o.t2 = o.rt1 = o.rt2 = 0.0f;
    const float id = p.idepth, x = p.u, y = p.v;
    const float rk0 = (w.RKi[0] * x + w.RKi[1] * y) + w.RKi[2] * 1.0f;
    const float rk1 = (w.RKi[3] * x + w.RKi[4] * y) + w.RKi[5] * 1.0f;
    const float rk2 = (w.RKi[6] * x + w.RKi[7] * y) + w.RKi[8] * 1.0f;
    const float pt0 = rk0 + w.t[0] * id, pt1 = rk1 + w.t[1] * id, pt2 = rk2 + w.t[2] * id;
    const float u = pt0 / pt2, v = pt1 / pt2;
    const float Ku = w.fx * u + w.cx, Kv = w.fy * v + w.cy;
    const float new_idepth = id / pt2;
    if (w.lvl == 0 && i % 32 == 0) {
        const float k0 = (w.fxi * x + 0.0f * y) + w.cxi * 1.0f, k1 = (0.0f * x + w.fyi * y) + w.cyi * 1.0f, k2 = (0.0f * x + 0.0f * y) + 1.0f * 1.0f;
        const float a0 = k0 + w.t[0] * id, a1 = k1 + w.t[1] * id, a2 = k2 + w.t[2] * id;
        const float KuT = w.fx * (a0 / a2) + w.cx, KvT = w.fy * (a1 / a2) + w.cy;
        const float b0 = k0 - w.t[0] * id, b1 = k1 - w.t[1] * id, b2 = k2 - w.t[2] * id;
        const float KuT2 = w.fx * (b0 / b2) + w.cx, KvT2 = w.fy * (b1 / b2) + w.cy;
        const float c0 = rk0 - w.t[0] * id, c1 = rk1 - w.t[1] * id, c2 = rk2 - w.t[2] * id;
        const float Ku3 = w.fx * (c0 / c2) + w.cx, Kv3 = w.fy * (c1 / c2) + w.cy;
        o.flow = 1;
        o.t1 = shift_sq(KuT, KvT, x, y); o.t2 = shift_sq(KuT2, KvT2, x, y);
        o.rt1 = shift_sq(Ku, Kv, x, y); o.rt2 = shift_sq(Ku3, Kv3, x, y);
    }
    if (!(Ku > 2 && Kv > 2 && Ku < w.wl3 && Kv < w.hl3 && new_idepth > 0)) return o;
    // getInterpolatedElement33
    const edsdso::Bilin bw = edsdso::bilin(Ku, Kv);
    const Px* bp = img + ((size_t)bw.iy * w.w + bw.ix);
    const Px v11 = bp[1 + w.w], v01 = bp[w.w], v10 = bp[1], v00 = bp[0];
    const float h0 = edsdso::mix(bw, v11.c, v01.c, v10.c, v00.c);
    const float h1 = edsdso::mix(bw, v11.dx, v01.dx, v10.dx, v00.dx);
    const float h2 = edsdso::mix(bw, v11.dy, v01.dy, v10.dy, v00.dy);
    if (!finite_f(h0)) return o;
    const float residual = h0 - (w.aff0 * p.color + w.aff1);
    const float ar = fabsf(residual);
    const float hw = ar < w.huber ? 1 : w.huber / ar;
    o.in_e = 1;
    if (ar > w.cutoff) { o.e = w.max_energy; return o; }
    o.e = hw * residual * residual * (2 - hw);
    o.warped = 1;
    o.idepth = new_idepth; o.u = u; o.v = v; o.dx = h1; o.dy = h2; o.residual = residual; o.weight = hw; o.ref_color = p.color;
    return o;
}

// rs[0 .. 5] of calcRes from the sums
EDS_HD void rs_from_sums(double E, int nE, int nSat, double sT, double sRT, int nFlow, double* rs) {
    const double num = 2.0 * nFlow;
    rs[0] = E; rs[1] = (double)nE; rs[2] = sT / (num + 0.1); rs[3] = 0.0; rs[4] = sRT / (num + 0.1);
    rs[5] = (double)((float)nSat / (float)nE);
}

// ---- calcGSSSE (CoarseTracker.cpp:287-344) ------------------------------------------------------------------------------------------
// J[0 .. 8] as the _mm_* calls nest them (J[7] = -1, J[8] = the residual), and the 45 products (J_a w) J_b, a <= b, row by row
EDS_HD void jacobian(const Warp& w, const Term& o, float* J) {
    const float dx = o.dx * w.fx, dy = o.dy * w.fy, u = o.u, v = o.v, id = o.idepth;
    J[0] = id * dx;
    J[1] = id * dy;
    J[2] = 0.0f - id * (u * dx + v * dy);
    J[3] = 0.0f - ((u * v) * dx + dy * (1.0f + v * v));
    J[4] = (u * v) * dy + dx * (1.0f + u * u);
    J[5] = u * dy - v * dx;
    J[6] = w.aff0 * (w.b0 - o.ref_color);
    J[7] = -1.0f;
    J[8] = o.residual;
}

// H (8 x 8, row-major) and b from the 45 sums and the number of warped rows; n is padded to a multiple of 4 as the reference's buffer is
EDS_HD double h_entry(const double* S, int n_warped, int r, int c) {
    const int n = (n_warped + 3) & ~3;
    const double inv = (double)(1.0f / (float)n);
    const int a = r < c ? r : c, b = r < c ? c : r;
    const int idx = a * 9 - a * (a - 1) / 2 + (b - a);
    const double sc = c == 6 ? 10.0 : c == 7 ? 1000.0 : 1.0, sr = r == 6 ? 10.0 : r == 7 ? 1000.0 : 1.0;
    if (c == 8) return (S[idx] * inv) * sr;                                      // b_out
    return ((S[idx] * inv) * sc) * sr;
}

// ---- the solve ----------------------------------------------------------------------------------------------------------------------
// unpivoted L D L^T of the leading N x N of the damped system (A's diagonal times `damp`, rhs = -b), then L z = rhs, y = z / d,
// L^T x = y.  STITCH: row and column 6 are A's row and column 7 and rhs[6] is -b[7] (the fixed-a case's HlStitch).
template <int N, bool STITCH>
EDS_HD void ldlt_solve(const double* A, const double* b, double damp, double* x) {
    double L[N][N], d[N], z[N];
#define EDS_CT_MAP(i) ((STITCH && (i) == 6) ? 7 : (i))
EDS_UNROLL
    for (int j = 0; j < N; ++j) {
        double dj = A[8 * EDS_CT_MAP(j) + EDS_CT_MAP(j)] * damp;
EDS_UNROLL
        for (int k = 0; k < j; ++k) dj -= (L[j][k] * L[j][k]) * d[k];
        d[j] = dj;
EDS_UNROLL
        for (int i = j + 1; i < N; ++i) {
            double v = A[8 * EDS_CT_MAP(i) + EDS_CT_MAP(j)];
EDS_UNROLL
            for (int k = 0; k < j; ++k) v -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = v / dj;
        }
    }
EDS_UNROLL
    for (int i = 0; i < N; ++i) {
        double v = -b[EDS_CT_MAP(i)];
EDS_UNROLL
        for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
        z[i] = v;
    }
#undef EDS_CT_MAP
EDS_UNROLL
    for (int i = 0; i < N; ++i) z[i] = z[i] / d[i];
EDS_UNROLL
    for (int i = N - 1; i >= 0; --i) {
        double v = z[i];
EDS_UNROLL
        for (int k = i + 1; k < N; ++k) v -= L[k][i] * x[k];
        x[i] = v;
    }
}

// the increment of one iteration: the damped system in the four affineOptMode cases (CoarseTracker.cpp:579-605)
EDS_HD void solve_inc(const double* H, const double* b, float lambda, const Params& s, double* inc) {
    double x[8];
    const double damp = (double)(1 + lambda);
EDS_UNROLL
    for (int i = 0; i < 8; ++i) x[i] = 0.0;
    const bool fix_a = s.affine_opt_mode_a < 0, fix_b = s.affine_opt_mode_b < 0;
    if (fix_a && fix_b) {
        ldlt_solve<6, false>(H, b, damp, x);
        x[6] = 0.0; x[7] = 0.0;
    } else if (fix_b) {
        ldlt_solve<7, false>(H, b, damp, x);
        x[7] = 0.0;
    } else if (fix_a) {
        ldlt_solve<7, true>(H, b, damp, x);
        x[7] = x[6]; x[6] = 0.0;
    } else {
        ldlt_solve<8, false>(H, b, damp, x);
    }
EDS_UNROLL
    for (int i = 0; i < 8; ++i) inc[i] = x[i];
}

// ---- SE3::exp(xi) * T (sophus/se3.hpp:406-428, so3.hpp:343-369) ---------------------------------------------------------------------
// xi = [upsilon, omega].  The pose is carried as R (row-major 3 x 3) and t: the product is R' = Rinc R, t' = Rinc t + V upsilon with
// Rinc the rotation matrix of the normalised quaternion, every 3-term sum left to right.
EDS_HD void se3_exp_mul(const double* xi, const double* R, const double* t, double* Rn, double* tn) {
    const double ox = xi[3], oy = xi[4], oz = xi[5];
    const double theta_sq = (ox * ox + oy * oy) + oz * oz;
    const double theta = sqrt(theta_sq), half = 0.5 * theta;
    double imag, real;
    const bool small_angle = theta < 1e-10;
    double sh = 0.0, ch = 1.0, st = 0.0, ct = 1.0;
    if (small_angle) {
        const double t4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * t4;
        real = 1.0 - 0.5 * theta_sq + (1.0 / 384.0) * t4;
    } else {
        sincos_d(half, &sh, &ch);
        sincos_d(theta, &st, &ct);
        imag = sh / theta; real = ch;
    }
    double qx = imag * ox, qy = imag * oy, qz = imag * oz, qw = real;
    const double qn = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
    qx = qx / qn; qy = qy / qn; qz = qz / qn; qw = qw / qn;
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const double Ri[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    const double Om[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double V[9];
    if (small_angle) {
EDS_UNROLL
        for (int i = 0; i < 9; ++i) V[i] = Ri[i];
    } else {
        const double c1 = (1.0 - ct) / theta_sq, c2 = (theta - st) / (theta_sq * theta);
EDS_UNROLL
        for (int i = 0; i < 3; ++i)
EDS_UNROLL
            for (int j = 0; j < 3; ++j) {
                const double o2 = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
                V[3 * i + j] = ((i == j ? 1.0 : 0.0) + c1 * Om[3 * i + j]) + c2 * o2;
            }
    }
EDS_UNROLL
    for (int i = 0; i < 3; ++i) {
EDS_UNROLL
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Ri[3 * i] * R[j] + Ri[3 * i + 1] * R[3 + j]) + Ri[3 * i + 2] * R[6 + j];
        const double rt = (Ri[3 * i] * t[0] + Ri[3 * i + 1] * t[1]) + Ri[3 * i + 2] * t[2];
        const double vu = (V[3 * i] * xi[0] + V[3 * i + 1] * xi[1]) + V[3 * i + 2] * xi[2];
        tn[i] = rt + vu;
    }
}

// ---- trackNewestCoarse (CoarseTracker.cpp:520-701) ----------------------------------------------------------------------------------
// Ev supplies calcRes's sums (res) and calcGSSSE's system (hess, then H() and b()); park / unpark bracket hess and may move the pose
// and rs out of registers while the 45 partials need them (the device keeps them in LDS; the host does nothing).  Every caller of one evaluator runs this on the same
// values; `writer` is the one that stores the result (thread 0 of the workgroup, or the host).  T is [R | t] row-major 3 x 4.
// fabsf(logf(x)) > 1.5 of the final affine check is restated without logf as x > e^1.5 or x < e^-1.5 (fp32 constants), NaN and
// negative x passing as they do in the reference.
template <class Ev>
EDS_HD void track(Ev& ev, const Params& s, const Photo& ph, const double* T_in, const double* aff_in, int coarsest, const double* min_res,
                     TrackOut* out, bool writer) {
    double R[9], t[3], a = aff_in[0], b = aff_in[1];
EDS_UNROLL
    for (int i = 0; i < 3; ++i) {
EDS_UNROLL
        for (int j = 0; j < 3; ++j) R[3 * i + j] = T_in[4 * i + j];
        t[i] = T_in[4 * i + 3];
    }
    if (writer) {
        for (int i = 0; i < 12; ++i) out->T[i] = T_in[i];
        out->aff[0] = aff_in[0]; out->aff[1] = aff_in[1];
        for (int i = 0; i < MAX_LEVELS; ++i) { out->last_residuals[i] = nan_d(); out->iters[i] = 0; out->accepts[i] = 0; }
        out->flow[0] = out->flow[1] = out->flow[2] = 1000.0;
        out->ok = 0; out->n_decisions = 0; out->cutoff_repeat = 1.0f; out->pad = 0;
    }
    const float limit = 0.001f;
    bool have_repeated = false;
    int nd = 0;
    for (int lvl = coarsest; lvl >= 0; --lvl) {
        float rep = 1;
        double rs_old[6], rs_new[6];
        ev.res(lvl, R, t, a, b, s.coarse_cutoff_th * rep, rs_old);
        while (rs_old[5] > 0.6 && rep < 50) {
            rep *= 2;
            ev.res(lvl, R, t, a, b, s.coarse_cutoff_th * rep, rs_old);
        }
        ev.park(R, t, rs_old);
        ev.hess(lvl, R, t, a, b, s.coarse_cutoff_th * rep);
        ev.unpark(R, t, rs_old);
        float lambda = 0.01f;
        const int max_it = lvl == 0 ? 10 : lvl == 1 ? 20 : 100;
        int its = 0, acc = 0;
        for (int it = 0; it < max_it; ++it) {
            double inc[8], incs[8], Rn[9], tn[3];
            solve_inc(ev.H(), ev.b(), lambda, s, inc);
            float extrap = 1;
            if (lambda < limit) extrap = sqrtf(sqrtf(limit / lambda));
            double sum = 0.0, sq = 0.0;
EDS_UNROLL
            for (int i = 0; i < 8; ++i) {
                inc[i] = inc[i] * (double)extrap;
                incs[i] = inc[i] * (i == 6 ? 10.0 : i == 7 ? 1000.0 : 1.0);
                sum += incs[i];
                sq += inc[i] * inc[i];
            }
            if (!finite_d(sum)) {
EDS_UNROLL
                for (int i = 0; i < 8; ++i) incs[i] = 0.0;
            }
            se3_exp_mul(incs, R, t, Rn, tn);
            const double an = a + incs[6], bn = b + incs[7];
            ev.res(lvl, Rn, tn, an, bn, s.coarse_cutoff_th * rep, rs_new);
            const bool accept = (rs_new[0] / rs_new[1]) < (rs_old[0] / rs_old[1]);
            if (writer && nd < MAX_DECISIONS) out->decisions[nd] = (uint8_t)((accept ? 1 : 0) | (lvl << 1));
            ++nd; ++its;
            if (accept) {
EDS_UNROLL
                for (int i = 0; i < 6; ++i) rs_old[i] = rs_new[i];
EDS_UNROLL
                for (int i = 0; i < 9; ++i) R[i] = Rn[i];
EDS_UNROLL
                for (int i = 0; i < 3; ++i) t[i] = tn[i];
                a = an; b = bn;
                lambda *= 0.5f;
                ++acc;
                ev.park(R, t, rs_old);
                ev.hess(lvl, R, t, a, b, s.coarse_cutoff_th * rep);     // the new pose's system, with only the accepted state live
                ev.unpark(R, t, rs_old);
            } else {
                lambda *= 4;
                if (lambda < limit) lambda = limit;
            }
            if (!(sqrt(sq) > 1e-3)) break;
        }
        const float last = sqrtf((float)(rs_old[0] / rs_old[1]));
        if (writer) {
            out->last_residuals[lvl] = (double)last;
            out->flow[0] = rs_old[2]; out->flow[1] = rs_old[3]; out->flow[2] = rs_old[4];
            out->iters[lvl] += its; out->accepts[lvl] += acc;
            out->cutoff_repeat = rep;
            out->n_decisions = nd < MAX_DECISIONS ? nd : MAX_DECISIONS;
        }
        if ((double)last > 1.5 * min_res[lvl]) return;                          // lastToNew_out and aff_g2l_out stay the inputs
        if (rep > 1 && !have_repeated) { ++lvl; have_repeated = true; }
    }
    if (writer) {
EDS_UNROLL
        for (int i = 0; i < 3; ++i) {
EDS_UNROLL
            for (int j = 0; j < 3; ++j) out->T[4 * i + j] = R[3 * i + j];
            out->T[4 * i + 3] = t[i];
        }
        out->aff[0] = a; out->aff[1] = b;
    }
    const float ma = s.affine_opt_mode_a, mb = s.affine_opt_mode_b;
    if ((ma != 0 && (double)fabsf((float)a) > 1.2) || (mb != 0 && fabsf((float)b) > 200)) return;
    double ra, rb;
    from_to_exposure(ph, a, b, &ra, &rb);
    const float rel0 = (float)ra, rel1 = (float)rb;
    if ((ma == 0 && (rel0 > 4.4816890703f || (rel0 < 0.2231301601f && rel0 >= 0.0f))) || (mb == 0 && fabsf(rel1) > 200)) return;
    if (writer) {
        if (ma < 0) out->aff[0] = 0.0;
        if (mb < 0) out->aff[1] = 0.0;
        out->ok = 1;
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the serial side: the same pieces walked in the device's order -------------------------------------------------------------------

// a frame's pyramid: px[g.total]
inline void make_pyramid(const Geo& g, const float* image, int64_t row_stride, Px* px) {
    Px* lv[MAX_LEVELS];
    for (int l = 0; l < g.levels; ++l) lv[l] = px + g.l[l].off;
    edsdso::make_levels(image, row_stride, g.W, g.H, g.levels, lv);
}

// makeCoarseDepthL0: idepth[g.total], wsum[g.total], pc[g.total] (a level's list starts at its off), pc_n[levels]; returns the dropped count
inline int make_depth(const Geo& g, const Px* ref, int n, const float* cp, const float* hdif, float* idepth, float* wsum, Pc* pc, int32_t* pc_n) {
    float* idA = new float[(size_t)g.total];
    float* wsA = new float[(size_t)g.total];
    for (int i = 0; i < g.total; ++i) { idA[i] = 0.0f; wsA[i] = 0.0f; }
    int dropped = 0;
    for (int i = 0; i < n; ++i) {
        int pix;
        if (!splat_pixel(cp[3 * i], cp[3 * i + 1], g.W, g.H, &pix)) { ++dropped; continue; }
        const float wgt = splat_weight(hdif[i]);
        idA[pix] += cp[3 * i + 2] * wgt;
        wsA[pix] += wgt;
    }
    for (int l = 1; l < g.levels; ++l) {
        const Level &L = g.l[l], &M = g.l[l - 1];
        for (int y = 0; y < L.h; ++y)
            for (int x = 0; x < L.w; ++x) {
                idA[L.off + x + y * L.w] = level_sum(idA + M.off, M.w, x, y);
                wsA[L.off + x + y * L.w] = level_sum(wsA + M.off, M.w, x, y);
            }
    }
    for (int l = 0; l < g.levels; ++l) {
        const Level& L = g.l[l];
        int cnt = 0;
        for (int i = 0; i < L.w * L.h; ++i) {
            float id, ws;
            dilate_at(idA + L.off, wsA + L.off, L.w, L.h, l, i, &id, &ws);
            const int x = i % L.w, y = i / L.w;
            const float color = ref[L.off + i].c;
            if (normalise_at(x, y, L.w, L.h, color, &id, &ws)) {
                Pc e = {(float)x, (float)y, id, color};
                pc[L.off + cnt++] = e;
            }
            idepth[L.off + i] = id; wsum[L.off + i] = ws;
        }
        pc_n[l] = cnt;
    }
    delete[] idA;
    delete[] wsA;
    return dropped;
}

struct SerialEval {
    const Geo* g; Params s; Photo ph;
    const Px* new_px; const Pc* pc; const int32_t* pc_n;
    double Hm[64], bv[8];
    int32_t n_warped;
    const double* H() const { return Hm; }
    const double* b() const { return bv; }
    void park(const double*, const double*, const double*) {}
    void unpark(double*, double*, double*) {}
    void res(int lvl, const double* R, const double* t, double a, double bb, float cutoff, double* rs) {
        const Level& L = g->l[lvl];
        const Warp w = make_warp(L, lvl, s, ph, R, t, a, bb, cutoff);
        double E[LANES] = {0}, sT[LANES] = {0}, sRT[LANES] = {0};
        int nE = 0, nSat = 0, nFlow = 0;
        for (int i = 0; i < pc_n[lvl]; ++i) {
            const Term o = point_term(w, new_px + L.off, pc[L.off + i], i);
            const int lane = i % LANES;
            if (o.flow) { sT[lane] += (double)o.t1; sT[lane] += (double)o.t2; sRT[lane] += (double)o.rt1; sRT[lane] += (double)o.rt2; ++nFlow; }
            if (o.in_e) { E[lane] += (double)o.e; ++nE; nSat += 1 - o.warped; }
        }
        rs_from_sums(reduce_lanes(E), nE, nSat, reduce_lanes(sT), reduce_lanes(sRT), nFlow, rs);
    }
    void hess(int lvl, const double* R, const double* t, double a, double bb, float cutoff) {
        const Level& L = g->l[lvl];
        const Warp w = make_warp(L, lvl, s, ph, R, t, a, bb, cutoff);
        static thread_local double part[NUM_SUMS][LANES];
        memset(part, 0, sizeof(part));
        int nW = 0;
        for (int i = 0; i < pc_n[lvl]; ++i) {
            const Term o = point_term(w, new_px + L.off, pc[L.off + i], i);
            if (!o.warped) continue;
            ++nW;
            float J[9];
            jacobian(w, o, J);
            int idx = 0;
            for (int r = 0; r < 9; ++r) {
                const float jw = J[r] * o.weight;
                for (int c = r; c < 9; ++c) part[idx++][i % LANES] += (double)(jw * J[c]);
            }
        }
        double S[NUM_SUMS];
        for (int q = 0; q < NUM_SUMS; ++q) S[q] = reduce_lanes(part[q]);
        for (int r = 0; r < 8; ++r) {
            for (int c = 0; c < 8; ++c) Hm[8 * r + c] = h_entry(S, nW, r, c);
            bv[r] = h_entry(S, nW, r, 8);
        }
        n_warped = nW;
    }
};

inline void track_serial(SerialEval& ev, const double* T_in, const double* aff_in, int coarsest, const double* min_res, TrackOut* out) {
    memset(out, 0, sizeof(*out));
    track(ev, ev.s, ev.ph, T_in, aff_in, coarsest, min_res, out, true);
}
#endif

}  // namespace edsct
