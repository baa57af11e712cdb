// DSO's window optimiser, the per-residual and per-point part (include/eds_hip_window.h): what the device kernels (eds_window.hip) and
// the host share — both projectPoint overloads, the geometric Jacobians, one tap of linearize's pattern loop, the ten running sums and
// the outlier rule, applyRes with takeDataF, the per-point sums of AccumulatedTopHessianSSE::addPoint<0> and the per-point prologue
// of AccumulatedSCHessianSSE::addPoint, every accumulator term of the two addPoint()s and both stitches — and a serial evaluator
// (linearize_serial, apply_serial, points_serial, accumulate_serial, stitch_serial) that strings them
// together in the reference's loop order.  fp32 per residual and per point in the reference's operand order; every translation unit
// that includes this is built without contraction into FMAs.  Plain C++ outside hipcc.  Level 0 of makeImages is edsdso's (one frame is
// one Px {c, dx, dy, 0} per pixel); nothing of it is written twice.
//
// WHAT J HOLDS AFTER AN OOB.  The reference leaves the RawResidualJacobian half-written when linearize returns OOB from inside the
// pattern loop.  Here a linearize that ends OOB — at entry, at the centre projection or at any tap — leaves EVERY word of the
// residual's J as the previous linearize left it (zeros before the first).  Nothing downstream reads it: applyRes copies J only for
// IN, and an OOB residual is never active again.  centerProjectedTo is written as soon as the centre projection passes, and
// projectedTo[k] for every tap k before the first failing one, and for the failing tap itself when it failed on a non-finite colour
// (its projection had passed), exactly as the reference's loop has written them when it returns; the other words keep their values.
//
// THE SUM ORDER.  The energy eds_win_linearize returns is the sum, in fp64, of the fp32 values linearize returns per residual, taken
// by LANES = 512 lanes: lane t adds, from 0.0, the returns of residuals t, t + 512, ... in that order; inside every 64 consecutive lanes
// the partials are folded by p[t] += p[t + s] for (t mod 64) < s, s = 32 ... 1; the eight totals are added left to right (edsdso's
// reduce_lanes).  Counts are integers.  No floating-point atomic anywhere.
#pragma once
#include "eds_dso_common.hpp"

namespace edswin {

using edsdso::finite_f;
using edsdso::Px;

constexpr int MAX_FRAMES = 8;
constexpr int PATTERN = 8;
using edsdso::LANES;
constexpr int J_WORDS = 74;
enum { ST_IN = 0, ST_OOB = 1, ST_OUTLIER = 2 };                 // ResState (Residuals.h:47)

// the words of one RawResidualJacobian, in the order eds_win_get_residuals returns them; the 2 x 2 blocks are row-major
enum { J_RESF = 0, J_JPDXI = 8, J_JPDC = 20, J_JPDD = 28, J_JIDX = 30, J_JABF = 46, J_JIDX2 = 62, J_JABJIDX = 66, J_JAB2 = 70 };

// eds_win_params, member for member
struct Params { float outlier_th_sum_component, huber_th, affine_opt_mode_a, affine_opt_mode_b, scale_idepth, scale_f, scale_c, reserved; };

struct Calib { float fx, fy, cx, cy, fxi, fyi, wM3, hM3; int32_t W, H; };

// one FrameFramePrecalc (HessianBlocks.cpp:204-234) as linearize reads it: 27 floats, matrices row-major
struct Precalc { float KRKi[9], Kt[3], R0[9], t0[3], aff[2], b0; };

// a point's constant part; its two inverse depths change every iteration and are arrays of their own (one plain copy per step)
struct Point { int32_t host; float u, v, color[PATTERN], weights[PATTERN]; };

EDS_HD int pat_x(int i) { const int t[PATTERN] = {0, -1, 1, -2, 0, 2, -1, 0}; return t[i]; }
EDS_HD int pat_y(int i) { const int t[PATTERN] = {-2, -1, -1, 0, 0, 0, 1, 2}; return t[i]; }

EDS_HD Params params_default() { Params p = {50.0f * 50.0f, 9.0f, 1e12f, 1e8f, 1.0f, 1.0f, 1.0f, 0.0f}; return p; }
EDS_HD bool params_valid(const Params& p) {
    return finite_f(p.outlier_th_sum_component) && finite_f(p.huber_th) && finite_f(p.affine_opt_mode_a) && finite_f(p.affine_opt_mode_b) &&
           finite_f(p.scale_idepth) && finite_f(p.scale_f) && finite_f(p.scale_c) && p.outlier_th_sum_component > 0.0f && p.huber_th > 0.0f &&
           p.scale_idepth > 0.0f && p.scale_f > 0.0f && p.scale_c > 0.0f;
}
EDS_HD bool shape_valid(int H, int W) { return H >= 8 && W >= 8 && H <= 8192 && W <= 8192; }

// CalibHessian's fxl() ... fyli() (HessianBlocks.h:350-366: value_scaledi[0] = 1 / fx) and globalCalib's wM3G, hM3G
EDS_HD Calib make_calib(int H, int W, float fx, float fy, float cx, float cy) {
    Calib c;
    c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.fxi = 1.0f / fx; c.fyi = 1.0f / fy;
    c.wM3 = (float)(W - 3); c.hM3 = (float)(H - 3); c.W = W; c.H = H;
    return c;
}

// ---- the geometric part of linearize (Residuals.cpp:94-148) with projectPoint's long overload (ResidualProjections.h:60-86) ------------
struct Geo { int32_t ok; float cp[3], Jpdxi[12], Jpdc[8], Jpdd[2]; };

EDS_HD Geo geo(const Calib& K, const Params& s, const Precalc& pc, float u_pt, float v_pt, float idepth_zero) {
    Geo g;
    g.ok = 0;
    g.cp[0] = g.cp[1] = g.cp[2] = 0.0f;
    for (int i = 0; i < 12; ++i) g.Jpdxi[i] = 0.0f;
    for (int i = 0; i < 8; ++i) g.Jpdc[i] = 0.0f;
    g.Jpdd[0] = g.Jpdd[1] = 0.0f;
    const float* R = pc.R0;
    const float* t = pc.t0;
    const float k0 = ((u_pt + 0.0f) - K.cx) * K.fxi, k1 = ((v_pt + 0.0f) - K.cy) * K.fyi;
    // R * KliP + t * idepth: every row of the product summed left to right, then the translation's term
    const float p0 = ((R[0] * k0 + R[1] * k1) + R[2] * 1.0f) + t[0] * idepth_zero;
    const float p1 = ((R[3] * k0 + R[4] * k1) + R[5] * 1.0f) + t[1] * idepth_zero;
    const float p2 = ((R[6] * k0 + R[7] * k1) + R[8] * 1.0f) + t[2] * idepth_zero;
    const float drescale = 1.0f / p2;
    const float new_idepth = idepth_zero * drescale;
    if (!(drescale > 0)) return g;
    const float u = p0 * drescale, v = p1 * drescale;
    const float Ku = u * K.fx + K.cx, Kv = v * K.fy + K.cy;
    if (!(Ku > 1.1f && Kv > 1.1f && Ku < K.wM3 && Kv < K.hM3)) return g;
    g.ok = 1;
    g.cp[0] = Ku; g.cp[1] = Kv; g.cp[2] = new_idepth;
    g.Jpdd[0] = ((drescale * (t[0] - t[2] * u)) * s.scale_idepth) * K.fx;
    g.Jpdd[1] = ((drescale * (t[1] - t[2] * v)) * s.scale_idepth) * K.fy;
    float cx2 = drescale * (R[6] * u - R[0]);
    float cx3 = ((K.fx * drescale) * (R[7] * u - R[1])) * K.fyi;
    float cx0 = k0 * cx2, cx1 = k1 * cx3;
    float cy2 = ((K.fy * drescale) * (R[6] * v - R[3])) * K.fxi;
    float cy3 = drescale * (R[7] * v - R[4]);
    float cy0 = k0 * cy2, cy1 = k1 * cy3;
    g.Jpdc[0] = (cx0 + u) * s.scale_f; g.Jpdc[1] = cx1 * s.scale_f; g.Jpdc[2] = (cx2 + 1) * s.scale_c; g.Jpdc[3] = cx3 * s.scale_c;
    g.Jpdc[4] = cy0 * s.scale_f; g.Jpdc[5] = (cy1 + v) * s.scale_f; g.Jpdc[6] = cy2 * s.scale_c; g.Jpdc[7] = (cy3 + 1) * s.scale_c;
    g.Jpdxi[0] = new_idepth * K.fx; g.Jpdxi[1] = 0.0f; g.Jpdxi[2] = ((-new_idepth) * u) * K.fx;
    g.Jpdxi[3] = ((-u) * v) * K.fx; g.Jpdxi[4] = (1 + u * u) * K.fx; g.Jpdxi[5] = (-v) * K.fx;
    g.Jpdxi[6] = 0.0f; g.Jpdxi[7] = new_idepth * K.fy; g.Jpdxi[8] = ((-new_idepth) * v) * K.fy;
    g.Jpdxi[9] = (-(1 + v * v)) * K.fy; g.Jpdxi[10] = (u * v) * K.fy; g.Jpdxi[11] = u * K.fy;
    return g;
}

// ---- one tap of the pattern loop (Residuals.cpp:174-236) ----------------------------------------------------------------------------------
// fail: 0 none, 1 the short projectPoint (:46-56) refused, 2 a non-finite colour.  s[0 .. 9]: the tap's addends to JIdxJIdx_00, _11,
// _10, JabJIdx_00, _01, _10, _11, JabJab_00, _01, _11.  No address is formed before the bounds test passes; a NaN fails it.
struct Tap { int32_t fail; float Ku, Kv, resF, jx, jy, ja, jb, e, wji2, s[10]; };

EDS_HD Tap tap(const Calib& K, const Params& s, const Precalc& pc, const Px* img, const Point& pt, float idepth_scaled, int idx) {
    Tap o;
    o.fail = 1;
    o.Ku = o.Kv = o.resF = o.jx = o.jy = o.ja = o.jb = o.e = o.wji2 = 0.0f;
    for (int i = 0; i < 10; ++i) o.s[i] = 0.0f;
    const float x = pt.u + (float)pat_x(idx), y = pt.v + (float)pat_y(idx), id = idepth_scaled;
    const float p0 = ((pc.KRKi[0] * x + pc.KRKi[1] * y) + pc.KRKi[2] * 1.0f) + pc.Kt[0] * id;
    const float p1 = ((pc.KRKi[3] * x + pc.KRKi[4] * y) + pc.KRKi[5] * 1.0f) + pc.Kt[1] * id;
    const float p2 = ((pc.KRKi[6] * x + pc.KRKi[7] * y) + pc.KRKi[8] * 1.0f) + pc.Kt[2] * id;
    const float Ku = p0 / p2, Kv = p1 / p2;
    if (!(Ku > 1.1f && Kv > 1.1f && Ku < K.wM3 && Kv < K.hM3)) return o;
    o.Ku = Ku; o.Kv = Kv;
    // getInterpolatedElement33 (globalFuncs.h:78-92)
    const edsdso::Bilin bw = edsdso::bilin(Ku, Kv);
    const Px* bp = img + ((size_t)bw.iy * K.W + bw.ix);
    const Px v11 = bp[1 + K.W], v01 = bp[K.W], v10 = bp[1], v00 = bp[0];
    const float h0 = edsdso::mix(bw, v11.c, v01.c, v10.c, v00.c);
    float h1 = edsdso::mix(bw, v11.dx, v01.dx, v10.dx, v00.dx);
    float h2 = edsdso::mix(bw, v11.dy, v01.dy, v10.dy, v00.dy);
    const float residual = h0 - (pc.aff[0] * pt.color[idx] + pc.aff[1]);
    const float drdA = pt.color[idx] - pc.b0;
    if (!finite_f(h0)) { o.fail = 2; return o; }
    o.fail = 0;
    float w = sqrtf(s.outlier_th_sum_component / (s.outlier_th_sum_component + (h1 * h1 + h2 * h2)));
    w = 0.5f * (w + pt.weights[idx]);
    float hw = fabsf(residual) < s.huber_th ? 1 : s.huber_th / fabsf(residual);
    o.e = w * w * hw * residual * residual * (2 - hw);
    if (hw < 1) hw = sqrtf(hw);
    hw = hw * w;
    h1 *= hw; h2 *= hw;
    o.resF = residual * hw;
    o.jx = h1; o.jy = h2; o.ja = drdA * hw; o.jb = hw;
    o.s[0] = h1 * h1; o.s[1] = h2 * h2; o.s[2] = h1 * h2;
    o.s[3] = drdA * hw * h1; o.s[4] = drdA * hw * h2; o.s[5] = hw * h1; o.s[6] = hw * h2;
    o.s[7] = drdA * drdA * hw * hw; o.s[8] = drdA * hw * hw; o.s[9] = hw * hw;
    o.wji2 = hw * hw * (h1 * h1 + h2 * h2);
    if (s.affine_opt_mode_a < 0) o.ja = 0.0f;
    if (s.affine_opt_mode_b < 0) o.jb = 0.0f;
    return o;
}

// the running sums of the loop, added in pattern order 0 ... 7 from 0: energyLeft, wJI2_sum and the ten products
struct Sums { float e, wji2, s[10]; };
EDS_HD Sums sums_zero() { Sums a; a.e = 0.0f; a.wji2 = 0.0f; for (int i = 0; i < 10; ++i) a.s[i] = 0.0f; return a; }
EDS_HD void sums_add(Sums& a, float e, float wji2, const float* s) {
    a.e += e; a.wji2 += wji2;
    for (int i = 0; i < 10; ++i) a.s[i] += s[i];
}

// the outlier rule (Residuals.cpp:251-263): std::max<float>(host, target) is (host < target) ? target : host
struct Verdict { int32_t state; float energy, energy_with_outlier; };
EDS_HD Verdict verdict(const Sums& a, float th_host, float th_target) {
    Verdict v;
    const float th = th_host < th_target ? th_target : th_host;
    v.energy_with_outlier = a.e;
    if (a.e > th || a.wji2 < 2) { v.energy = th; v.state = ST_OUTLIER; }
    else { v.energy = a.e; v.state = ST_IN; }
    return v;
}

// the twelve words of JIdx2, JabJIdx and Jab2 (row-major 2 x 2 each) from the sums (Residuals.cpp:238-249)
EDS_HD float block_word(const Sums& a, int k) {
    const int m[12] = {0, 2, 2, 1, 3, 4, 5, 6, 7, 8, 8, 9};
    return a.s[m[k]];
}

// ---- applyRes (Residuals.cpp:298-320) with EFResidual::takeDataF (EnergyFunctionalStructs.cpp:38-48) ---------------------------------------
// JpJdF from a J: JI_JI_Jd = JIdx2 * Jpdd, JpJdF[i] = Jpdxi[0][i] JI_JI_Jd[0] + Jpdxi[1][i] JI_JI_Jd[1], JpJdF[6 .. 7] = JabJIdx * Jpdd
EDS_HD void jpjdf(const float* J, float* out) {
    const float d0 = J[J_JPDD], d1 = J[J_JPDD + 1];
    const float a = J[J_JIDX2] * d0 + J[J_JIDX2 + 1] * d1, b = J[J_JIDX2 + 2] * d0 + J[J_JIDX2 + 3] * d1;
    for (int i = 0; i < 6; ++i) out[i] = J[J_JPDXI + i] * a + J[J_JPDXI + 6 + i] * b;
    out[6] = J[J_JABJIDX] * d0 + J[J_JABJIDX + 1] * d1;
    out[7] = J[J_JABJIDX + 2] * d0 + J[J_JABJIDX + 3] * d1;
}

// one residual's applyRes.  takeDataF swaps two J pointers; here the linearized J is COPIED into the energy functional's, which gives the
// functional the same words (the swapped-out buffer is overwritten by the next linearize that does not end OOB, and read by nothing).
struct ResState { int32_t* state; float* energy; int32_t* active; const int32_t* new_state; const float* new_energy; const float* J; float* efJ; float* JpJdF; };
EDS_HD void apply_one(const ResState& r, int i, bool copy_jacobians) {
    if (copy_jacobians) {
        if (r.state[i] == ST_OOB) return;                       // can never go back from OOB
        if (r.new_state[i] == ST_IN) {
            r.active[i] = 1;
            for (int k = 0; k < J_WORDS; ++k) r.efJ[(size_t)i * J_WORDS + k] = r.J[(size_t)i * J_WORDS + k];
            jpjdf(r.efJ + (size_t)i * J_WORDS, r.JpJdF + (size_t)i * 8);
        } else {
            r.active[i] = 0;
        }
    }
    r.state[i] = r.new_state[i];
    r.energy[i] = r.new_energy[i];
}

// ---- per point: AccumulatedTopHessianSSE::addPoint<0> (AccumulatedTopHessian.cpp:49-145) and the prologue of the Schur complement's
// addPoint (AccumulatedSCHessian.cpp:36-55), residuals in residualsAll order = the order of the residual table -----------------------------
struct PointOut { float Hdd_accAF, bd_accAF, Hcd_accAF[4], HdiF, bdSumF, idepth_hessian; int32_t nres; };

// Mode 0 of the top accumulator skips residuals with isLinearized while the Schur complement's ngoodres counts every active one.  The
// flags live beside the table (lin[r], NULL: none is set; include/eds_hip_winsolve.h sets them); PointOut::nres is ngoodres.
// One residual's addends to bd_acc, Hdd_acc and Hcd_acc (AccumulatedTopHessian.cpp:102-137); res: the eight words of resApprox
EDS_HD void top_point_term(const float* J, const float* res, float& bd, float& Hdd, float* Hcd) {
    float jr0 = 0, jr1 = 0;
    for (int i = 0; i < PATTERN; ++i) {
        jr0 += res[i] * J[J_JIDX + i];
        jr1 += res[i] * J[J_JIDX + 8 + i];
    }
    const float d0 = J[J_JPDD], d1 = J[J_JPDD + 1];
    const float q0 = J[J_JIDX2] * d0 + J[J_JIDX2 + 1] * d1, q1 = J[J_JIDX2 + 2] * d0 + J[J_JIDX2 + 3] * d1;
    bd += jr0 * d0 + jr1 * d1;
    Hdd += q0 * d0 + q1 * d1;
    for (int k = 0; k < 4; ++k) Hcd[k] += J[J_JPDC + k] * q0 + J[J_JPDC + 4 + k] * q1;
}
// the residual filter of addPoint<mode>: 0 active and not linearized, 1 active and linearized, 2 active
EDS_HD bool top_filter(int mode, int is_active, int is_lin) { return is_active && (mode == 2 || (mode == 1) == (is_lin != 0)); }

// the point's residuals are [r0, r1) of the table; prior, delta and the linearized sums Hdd_accLF, bd_accLF, Hcd_accLF[4] are inputs.
// mode 0: the A sums over the residuals that are active and not linearized; mode 2: the A sums are zero (addPoint<2> zeroes them)
EDS_HD PointOut point_sums_mode(const int32_t* active, const int32_t* lin, const float* efJ, int r0, int r1, float priorF, float deltaF,
                                    const float* lf, bool shift_prior_to_zero, int mode, int* added) {
    PointOut o;
    float bd = 0, Hdd = 0, Hcd[4] = {0, 0, 0, 0};
    int n = 0, na = 0;
    for (int r = r0; r < r1; ++r) {
        if (!active[r]) continue;
        ++n;
        if (mode != 0 || (lin && lin[r])) continue;
        const float* J = efJ + (size_t)r * J_WORDS;
        top_point_term(J, J + J_RESF, bd, Hdd, Hcd);
        ++na;
    }
    *added = na;
    o.Hdd_accAF = Hdd; o.bd_accAF = bd; o.nres = n;
    for (int k = 0; k < 4; ++k) o.Hcd_accAF[k] = Hcd[k];
    if (n == 0) { o.HdiF = 0.0f; o.bdSumF = 0.0f; o.idepth_hessian = 0.0f; return o; }
    float H = Hdd + lf[0] + priorF;
    if (H < 1e-10) H = (float)1e-10;
    o.idepth_hessian = H;
    o.HdiF = (float)(1.0 / H);
    o.bdSumF = bd + lf[1];
    if (shift_prior_to_zero) o.bdSumF += priorF * deltaF;
    return o;
}
EDS_HD PointOut point_sums(const int32_t* active, const float* efJ, int r0, int r1, float priorF, float deltaF, const float* lf,
                               bool shift_prior_to_zero) {
    int added;
    return point_sums_mode(active, nullptr, efJ, r0, r1, priorF, deltaF, lf, shift_prior_to_zero, 0, &added);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the serial side ---------------------------------------------------------------------------------------------------------------------
struct Tables {
    int m;
    const int32_t* res_point; const int32_t* res_target;
    int32_t *state, *new_state, *active;
    float *energy, *new_energy, *new_energy_wo, *ret, *cp, *proj, *J, *efJ, *JpJdF;
};

// one frame's level 0: px[H * W]
inline void make_frame(int H, int W, const float* image, int64_t row_stride, Px* px) { edsdso::make_levels(image, row_stride, W, H, 1, &px); }

// PointFrameResidual::linearize for residual i; returns what the reference returns
inline float linearize_one(const Calib& K, const Params& s, int F, const Precalc* pcs, const float* th, const Px* frames, const Point* pts,
                           const float* ids, const float* idz, const Tables& t, int i) {
    t.new_energy_wo[i] = -1.0f;
    if (t.state[i] == ST_OOB) { t.new_state[i] = ST_OOB; return t.energy[i]; }
    const Point& pt = pts[t.res_point[i]];
    const int tg = t.res_target[i];
    const Precalc& pc = pcs[pt.host * F + tg];
    const Geo g = geo(K, s, pc, pt.u, pt.v, idz[t.res_point[i]]);
    if (!g.ok) { t.new_state[i] = ST_OOB; return t.energy[i]; }
    for (int k = 0; k < 3; ++k) t.cp[(size_t)i * 3 + k] = g.cp[k];
    Tap taps[PATTERN];
    Sums a = sums_zero();
    for (int k = 0; k < PATTERN; ++k) {
        taps[k] = tap(K, s, pc, frames + (size_t)tg * K.W * K.H, pt, ids[t.res_point[i]], k);
        if (taps[k].fail != 1) { t.proj[(size_t)i * 16 + 2 * k] = taps[k].Ku; t.proj[(size_t)i * 16 + 2 * k + 1] = taps[k].Kv; }
        if (taps[k].fail) { t.new_state[i] = ST_OOB; return t.energy[i]; }
        sums_add(a, taps[k].e, taps[k].wji2, taps[k].s);
    }
    float* J = t.J + (size_t)i * J_WORDS;
    for (int k = 0; k < PATTERN; ++k) {
        J[J_RESF + k] = taps[k].resF; J[J_JIDX + k] = taps[k].jx; J[J_JIDX + 8 + k] = taps[k].jy;
        J[J_JABF + k] = taps[k].ja; J[J_JABF + 8 + k] = taps[k].jb;
    }
    for (int k = 0; k < 12; ++k) J[J_JPDXI + k] = g.Jpdxi[k];
    for (int k = 0; k < 8; ++k) J[J_JPDC + k] = g.Jpdc[k];
    J[J_JPDD] = g.Jpdd[0]; J[J_JPDD + 1] = g.Jpdd[1];
    for (int k = 0; k < 12; ++k) J[J_JIDX2 + k] = block_word(a, k);
    const Verdict v = verdict(a, th[pt.host], th[tg]);
    t.new_energy_wo[i] = v.energy_with_outlier;
    t.new_state[i] = v.state;
    t.new_energy[i] = v.energy;
    return v.energy;
}

// every residual, then the energy in the header's sum order and the counts of the new states {IN, OOB, OUTLIER}
inline double linearize_serial(const Calib& K, const Params& s, int F, const Precalc* pcs, const float* th, const Px* frames, const Point* pts,
                               const float* ids, const float* idz, const Tables& t, int32_t* counts) {
    double part[LANES];
    for (int l = 0; l < LANES; ++l) part[l] = 0.0;
    counts[0] = counts[1] = counts[2] = 0;
    for (int i = 0; i < t.m; ++i) {
        t.ret[i] = linearize_one(K, s, F, pcs, th, frames, pts, ids, idz, t, i);
        part[i % LANES] += (double)t.ret[i];
        ++counts[t.new_state[i]];
    }
    return edsdso::reduce_lanes(part);
}

inline void apply_serial(const Tables& t, bool copy_jacobians) {
    const ResState r = {t.state, t.energy, t.active, t.new_state, t.new_energy, t.J, t.efJ, t.JpJdF};
    for (int i = 0; i < t.m; ++i) apply_one(r, i, copy_jacobians);
}

// res_first[p] .. res_first[p + 1]: point p's residuals; returns nres, the active residuals added
inline int points_serial(int n, const int32_t* res_first, const Tables& t, const float* priorF, const float* deltaF, const float* lf,
                         bool shift_prior_to_zero, PointOut* out) {
    const float zero[6] = {0, 0, 0, 0, 0, 0};
    int nres = 0;
    for (int p = 0; p < n; ++p) {
        out[p] = point_sums(t.active, t.efJ, res_first[p], res_first[p + 1], priorF ? priorF[p] : 0.0f, deltaF ? deltaF[p] : 0.0f,
                            lf ? lf + 6 * p : zero, shift_prior_to_zero);
        nres += out[p].nres;
    }
    return nres;
}
#endif

// ---- the accumulators of the two addPoint()s and both stitches -------------------------------------------------------------------------
// THE ACCUMULATOR SUM ORDER.  Every accumulator entry is a sum over the POINTS of one host frame (an accumulator acc[h + F t],
// accE / accEB[h + F t] or accD[h + F t1 + F^2 t2] has contributions from host h only; accHcc / accbc from every host).  Every term is
// the reference's fp32 value, widened to fp64; a point that does not contribute (no active residual towards that target) adds +0.0, so
// nothing is compacted.  LANES = 512 lanes stride the point index WITHIN the host frame (lane = (p - first point of the host) mod 512),
// each adding from 0.0 in index order; inside every 64 lanes p[t] += p[t + s], s = 32 ... 1; the eight totals left to right
// (reduce_lanes); for accHcc / accbc the F host totals are then added left to right, hosts 0 ... F - 1.  Counts (num) are sums of 1.0
// and exact.  A point has at most one residual per target (eds_win_accumulate refuses anything else).
//
// One flat array of doubles holds everything, acc_size(F) long:
//   top  [F F][92]  entry e < 55: Data[e] of AccumulatorApprox::update (MatrixAccumulators.h:764-841), 55 + 3 k + q: TopRight_Data,
//                   85 ... 90: BotRight_Data, 91: num
//   E    [F F][40]  accE (8 x 4 row-major), then accEB (8)
//   D    [F F F][65] accD[h + F t1 + F^2 t2] (8 x 8 row-major), then num
//   C    [F][20]    per host: accHcc (4 x 4 row-major), then accbc (4)
constexpr int TOP_WORDS = 92, E_WORDS = 40, D_WORDS = 65, C_WORDS = 20;
EDS_HD int acc_off_e(int F) { return F * F * TOP_WORDS; }
EDS_HD int acc_off_d(int F) { return acc_off_e(F) + F * F * E_WORDS; }
EDS_HD int acc_off_c(int F) { return acc_off_d(F) + F * F * F * D_WORDS; }
EDS_HD int acc_size(int F) { return acc_off_c(F) + F * C_WORDS; }

// x4 | x6 and y4 | y6 of the update calls: Jpdc[0], Jpdxi[0] and Jpdc[1], Jpdxi[1]
EDS_HD float jx(const float* J, int k) { return k < 4 ? J[J_JPDC + k] : J[J_JPDXI + k - 4]; }
EDS_HD float jy(const float* J, int k) { return k < 4 ? J[J_JPDC + 4 + k] : J[J_JPDXI + 6 + k - 4]; }
// sum_i a[i] b[i] from 0 in index order (JI_r, Jab_r, rr of AccumulatedTopHessian.cpp:102-112)
EDS_HD float dot8(const float* a, const float* b) { float r = 0; for (int i = 0; i < PATTERN; ++i) r += a[i] * b[i]; return r; }

// entry e of what one active residual adds to acc[h + F t] (AccumulatedTopHessian.cpp:115-129); res: the eight words of resApprox (mode 0:
// the J's own resF)
EDS_HD float top_term(const float* J, const float* res, int e) {
    if (e < 55) {                                               // Data: column c, rows r = c ... 9
        int c = 0, base = 0;
        while (e >= base + (10 - c)) { base += 10 - c; ++c; }
        const int r = c + (e - base);
        const float a = J[J_JIDX2], b = J[J_JIDX2 + 1], cc = J[J_JIDX2 + 3];
        const float xr = jx(J, r), xc = jx(J, c), yr = jy(J, r), yc = jy(J, c);
        return a * xr * xc + cc * yr * yc + b * (xr * yc + yr * xc);
    }
    if (e < 85) {                                               // TopRight: x TR0q + y TR1q
        const int k = (e - 55) / 3, q = (e - 55) % 3;
        const float t0 = q == 0 ? J[J_JABJIDX] : q == 1 ? J[J_JABJIDX + 2] : dot8(res, J + J_JIDX);
        const float t1 = q == 0 ? J[J_JABJIDX + 1] : q == 1 ? J[J_JABJIDX + 3] : dot8(res, J + J_JIDX + 8);
        return jx(J, k) * t0 + jy(J, k) * t1;
    }
    switch (e) {
        case 85: return J[J_JAB2];
        case 86: return J[J_JAB2 + 1];
        case 87: return dot8(res, J + J_JABF);
        case 88: return J[J_JAB2 + 3];
        case 89: return dot8(res, J + J_JABF + 8);
        case 90: return dot8(res, res);
        default: return 1.0f;
    }
}
EDS_HD float top_term(const float* J, int e) { return top_term(J, J + J_RESF, e); }

// what a term reads; res_of[p F + t]: the residual of point p towards target t, or -1
// The trailing members are zero in every brace list that ends at lf: mode 0, no linearized flag, every point.  lin[r]: isLinearized;
// res_approx[r][8]: resApprox of modes 1 and 2; sel[p]: only the points with sel[p] != 0 contribute (marginalisation)
struct AccIn { int32_t F, has_lf; const int32_t* first; const int32_t* res_of; const int32_t* active; const float* efJ; const float* JpJdF; const PointOut* pout; const float* lf;
               int32_t mode; const int32_t* lin; const float* res_approx; const int32_t* sel; };

EDS_HD int active_res(const AccIn& in, int p, int t) {
    const int r = in.res_of[p * in.F + t];
    return r >= 0 && in.active[r] ? r : -1;
}
// the residual of point p towards target t that addPoint<mode> of the top accumulator takes, or -1
EDS_HD int top_res(const AccIn& in, int p, int t) {
    const int r = in.res_of[p * in.F + t];
    return r >= 0 && top_filter(in.mode, in.active[r], in.lin ? in.lin[r] : 0) ? r : -1;
}
// Hcd = Hcd_accAF + Hcd_accLF (AccumulatedSCHessian.cpp:55)
EDS_HD float hcd(const AccIn& in, int p, int k) { return in.pout[p].Hcd_accAF[k] + (in.has_lf ? in.lf[6 * p + 2 + k] : 0.0f); }

// the host frame of accumulator word j, and what point p adds to it.  AccumulatorXX::update(L, R, w) adds (w L[i]) R[j],
// AccumulatorX::update(L, w) adds w L[i] (MatrixAccumulators.h); the weights are HdiF, bdSumF * HdiF (accbc) and HdiF * bdSumF (accEB).
EDS_HD int acc_host(int F, int j) {
    if (j < acc_off_e(F)) return (j / TOP_WORDS) % F;
    if (j < acc_off_d(F)) return ((j - acc_off_e(F)) / E_WORDS) % F;
    if (j < acc_off_c(F)) return ((j - acc_off_d(F)) / D_WORDS) % F;
    return (j - acc_off_c(F)) / C_WORDS;
}
EDS_HD double acc_value(const AccIn& in, int j, int p) {
    const int F = in.F;
    if (in.sel && !in.sel[p]) return 0.0;
    if (j < acc_off_e(F)) {
        const int r = top_res(in, p, (j / TOP_WORDS) / F);
        if (r < 0) return 0.0;
        const float* J = in.efJ + (size_t)r * J_WORDS;
        return (double)top_term(J, in.mode == 0 ? J + J_RESF : in.res_approx + (size_t)r * PATTERN, j % TOP_WORDS);
    }
    if (j < acc_off_d(F)) {
        const int q = j - acc_off_e(F), e = q % E_WORDS, r = active_res(in, p, (q / E_WORDS) / F);
        if (r < 0) return 0.0;
        const float* Jp = in.JpJdF + (size_t)r * 8;
        const float hdi = in.pout[p].HdiF;
        if (e < 32) return (double)((hdi * Jp[e / 4]) * hcd(in, p, e % 4));
        return (double)((hdi * in.pout[p].bdSumF) * Jp[e - 32]);
    }
    if (j < acc_off_c(F)) {
        const int q = j - acc_off_d(F), e = q % D_WORDS, a = q / D_WORDS;
        const int r1 = active_res(in, p, (a / F) % F), r2 = active_res(in, p, a / (F * F));
        if (r1 < 0 || r2 < 0) return 0.0;
        if (e == 64) return 1.0;
        return (double)((in.pout[p].HdiF * in.JpJdF[(size_t)r1 * 8 + e / 8]) * in.JpJdF[(size_t)r2 * 8 + e % 8]);
    }
    const int e = (j - acc_off_c(F)) % C_WORDS;
    if (in.pout[p].nres == 0) return 0.0;
    const float hdi = in.pout[p].HdiF;
    if (e < 16) return (double)((hdi * hcd(in, p, e / 4)) * hcd(in, p, e % 4));
    return (double)((in.pout[p].bdSumF * hdi) * hcd(in, p, e - 16));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// every accumulator word in the order above
inline void accumulate_serial(const AccIn& in, double* acc) {
    const int n = acc_size(in.F);
    for (int j = 0; j < n; ++j) {
        const int h = acc_host(in.F, j);
        double part[LANES];
        for (int l = 0; l < LANES; ++l) part[l] = 0.0;
        for (int p = in.first[h]; p < in.first[h + 1]; ++p) part[(p - in.first[h]) % LANES] += acc_value(in, j, p);
        acc[j] = edsdso::reduce_lanes(part);
    }
}

#endif

// ---- the stitches, fp64, every sum from 0.0 in index order --------------------------------------------------------------------------------
// A (8 x 8) times M (8 x cols, row stride ms), row-major: out(r, c) = sum_l A(r, l) M(l, c), l = 0 ... 7 left to right
inline void mul8(const double* A, const double* M, int ms, int cols, double* out) {
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < cols; ++c) { double v = 0.0; for (int l = 0; l < 8; ++l) v += A[8 * r + l] * M[ms * l + c]; out[cols * r + c] = v; }
}
// (A M) B^T: first T = A M by mul8, then out(r, c) = sum_k T(r, k) B(c, k), k = 0 ... 7 left to right
inline void triple8(const double* A, const double* M, int ms, const double* B, double* out) {
    double T[64];
    mul8(A, M, ms, 8, T);
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) { double v = 0.0; for (int k = 0; k < 8; ++k) v += T[8 * r + k] * B[8 * c + k]; out[8 * r + c] = v; }
}
inline void add_block(double* H, int N, int i0, int j0, const double* blk, int rows, int cols) {
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) H[(size_t)(i0 + r) * N + j0 + c] += blk[cols * r + c];
}
// the 13 x 13 H of AccumulatorApprox::finish from 91 words
inline void top_h13(const double* w, double* H) {
    int idx = 0;
    for (int r = 0; r < 10; ++r) for (int c = r; c < 10; ++c) { H[13 * r + c] = H[13 * c + r] = w[idx]; ++idx; }
    for (int r = 0; r < 10; ++r) for (int c = 0; c < 3; ++c) H[13 * r + c + 10] = H[13 * (c + 10) + r] = w[55 + 3 * r + c];
    H[13 * 10 + 10] = w[85]; H[13 * 10 + 11] = H[13 * 11 + 10] = w[86]; H[13 * 10 + 12] = H[13 * 12 + 10] = w[87];
    H[13 * 11 + 11] = w[88]; H[13 * 11 + 12] = H[13 * 12 + 11] = w[89]; H[13 * 12 + 12] = w[90];
}

// AccumulatedTopHessianSSE::stitchDouble with usePrior = false (AccumulatedTopHessian.cpp:171-225) and AccumulatedSCHessianSSE::stitchDouble
// (AccumulatedSCHessian.cpp:159-219), block sums in the reference's loop and statement order; adH / adT: [h + F t][8][8] row-major;
// H_A, H_sc: N x N row-major, N = 4 + 8 F.  The priors of usePrior are a diagonal add and stay with the caller.
inline void stitch_serial(int F, const double* acc, const double* adH, const double* adT, double* HA, double* bA, double* Hsc, double* bsc) {
    const int N = 4 + 8 * F;
    for (int i = 0; i < N * N; ++i) { HA[i] = 0.0; Hsc[i] = 0.0; }
    for (int i = 0; i < N; ++i) { bA[i] = 0.0; bsc[i] = 0.0; }
    double blk[64], H13[169];
    for (int h = 0; h < F; ++h)
        for (int t = 0; t < F; ++t) {
            const int a = h + F * t, hI = 4 + 8 * h, tI = 4 + 8 * t;
            const double* w = acc + (size_t)a * TOP_WORDS;
            if (w[91] == 0.0) continue;                          // num == 0
            top_h13(w, H13);
            const double *AH = adH + 64 * a, *AT = adT + 64 * a, *M88 = H13 + 13 * 4 + 4, *M84 = H13 + 13 * 4, *v8 = H13 + 13 * 4 + 12;
            triple8(AH, M88, 13, AH, blk); add_block(HA, N, hI, hI, blk, 8, 8);
            triple8(AT, M88, 13, AT, blk); add_block(HA, N, tI, tI, blk, 8, 8);
            triple8(AH, M88, 13, AT, blk); add_block(HA, N, hI, tI, blk, 8, 8);
            mul8(AH, M84, 13, 4, blk); add_block(HA, N, hI, 0, blk, 8, 4);
            mul8(AT, M84, 13, 4, blk); add_block(HA, N, tI, 0, blk, 8, 4);
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) HA[(size_t)r * N + c] += H13[13 * r + c];
            mul8(AH, v8, 13, 1, blk); for (int r = 0; r < 8; ++r) bA[hI + r] += blk[r];
            mul8(AT, v8, 13, 1, blk); for (int r = 0; r < 8; ++r) bA[tI + r] += blk[r];
            for (int r = 0; r < 4; ++r) bA[r] += H13[13 * r + 12];
        }
    for (int h = 0; h < F; ++h) {                               // the transposed copies
        const int hI = 4 + 8 * h;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 8; ++c) HA[(size_t)r * N + hI + c] = HA[(size_t)(hI + c) * N + r];
        for (int t = h + 1; t < F; ++t) {
            const int tI = 4 + 8 * t;
            for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) HA[(size_t)(hI + r) * N + tI + c] += HA[(size_t)(tI + c) * N + hI + r];
            for (int r = 0; r < 8; ++r) for (int c = 0; c < 8; ++c) HA[(size_t)(tI + r) * N + hI + c] = HA[(size_t)(hI + c) * N + tI + r];
        }
    }
    double M[64];
    for (int i = 0; i < F; ++i)
        for (int j = 0; j < F; ++j) {
            const int ij = i + F * j, iI = 4 + 8 * i, jI = 4 + 8 * j;
            const double* E = acc + acc_off_e(F) + (size_t)ij * E_WORDS;
            mul8(adH + 64 * ij, E, 4, 4, blk); add_block(Hsc, N, iI, 0, blk, 8, 4);
            mul8(adT + 64 * ij, E, 4, 4, blk); add_block(Hsc, N, jI, 0, blk, 8, 4);
            mul8(adH + 64 * ij, E + 32, 1, 1, blk); for (int r = 0; r < 8; ++r) bsc[iI + r] += blk[r];
            mul8(adT + 64 * ij, E + 32, 1, 1, blk); for (int r = 0; r < 8; ++r) bsc[jI + r] += blk[r];
            for (int k = 0; k < F; ++k) {
                const int kI = 4 + 8 * k, ik = i + F * k;
                const double* D = acc + acc_off_d(F) + (size_t)(ij + k * F * F) * D_WORDS;
                if (D[64] == 0.0) continue;                      // num == 0
                for (int q = 0; q < 64; ++q) M[q] = D[q];
                triple8(adH + 64 * ij, M, 8, adH + 64 * ik, blk); add_block(Hsc, N, iI, iI, blk, 8, 8);
                triple8(adT + 64 * ij, M, 8, adT + 64 * ik, blk); add_block(Hsc, N, jI, kI, blk, 8, 8);
                triple8(adT + 64 * ij, M, 8, adH + 64 * ik, blk); add_block(Hsc, N, jI, iI, blk, 8, 8);
                triple8(adH + 64 * ij, M, 8, adT + 64 * ik, blk); add_block(Hsc, N, iI, kI, blk, 8, 8);
            }
        }
    const double* C = acc + acc_off_c(F);
    for (int e = 0; e < 20; ++e) {                              // hosts 0 ... F - 1 left to right
        double v = 0.0;
        for (int h = 0; h < F; ++h) v += C[h * C_WORDS + e];
        if (e < 16) Hsc[(size_t)(e / 4) * N + e % 4] = v; else bsc[e - 16] = v;
    }
    for (int h = 0; h < F; ++h)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 8; ++c) Hsc[(size_t)r * N + 4 + 8 * h + c] = Hsc[(size_t)(4 + 8 * h + c) * N + r];
}

// ---- the same stitches, one output entry at a time (what k_win_stitch runs, one thread per entry) ------------------------------------------
// Every entry receives the same addends in the same order as in stitch_serial: a block product's entry is sum_k (sum_l A(r,l) M(l,k)) B(c,k)
// with both sums from 0.0 left to right, and the products are added into the entry in the loop and statement order of the reference.
// entry (r, c) of the 13 x 13 H of AccumulatorApprox::finish, straight from the 91 words
EDS_HD double h13_at(const double* w, int r, int c) {
    const int a = r < c ? r : c, b = r < c ? c : r;
    if (b < 10) return w[a * 10 - a * (a - 1) / 2 + (b - a)];
    if (a < 10) return w[55 + 3 * a + (b - 10)];
    return w[a == 10 ? 85 + (b - 10) : a == 11 ? 88 + (b - 11) : 90];
}
// sum_l A(r, l) M(l, c) with M given by a word array and a (row, column) -> word rule: kind 0 the 13 x 13 H at offset (4 + l, c0 + c),
// kind 1 a dense row-major matrix with `ms` columns
EDS_HD double m_at(const double* w, int kind, int ms, int c0, int l, int c) { return kind == 0 ? h13_at(w, 4 + l, c0 + c) : w[ms * l + c]; }
EDS_HD double row_dot(const double* A, int r, const double* w, int kind, int ms, int c0, int c) {
    double v = 0.0;
    for (int l = 0; l < 8; ++l) v += A[8 * r + l] * m_at(w, kind, ms, c0, l, c);
    return v;
}
EDS_HD double tri_at(const double* A, const double* w, int kind, int ms, int c0, const double* B, int r, int c) {
    double v = 0.0;
    for (int k = 0; k < 8; ++k) v += row_dot(A, r, w, kind, ms, c0, k) * B[8 * c + k];
    return v;
}
// H_A before the transposed copies: i a pose row or a calibration row, j a column or N for b; only the entries the accumulation writes
EDS_HD double top_raw(int F, const double* acc, const double* adH, const double* adT, int i, int j) {
    const int N = 4 + 8 * F;
    const bool pi = i >= 4, pj = j >= 4 && j < N;
    const int I = pi ? (i - 4) / 8 : -1, r = pi ? (i - 4) % 8 : i, J = pj ? (j - 4) / 8 : -1, c = pj ? (j - 4) % 8 : j;
    double v = 0.0;
    for (int h = 0; h < F; ++h)
        for (int t = 0; t < F; ++t) {
            if (pi && I != h && I != t) continue;                // this pair adds nothing to a row of block I
            const int a = h + F * t;
            const double* w = acc + (size_t)a * TOP_WORDS;
            if (w[91] == 0.0) continue;
            const double *AH = adH + 64 * a, *AT = adT + 64 * a;
            if (pi && pj) {
                if (I == h && J == h) v += tri_at(AH, w, 0, 0, 4, AH, r, c);
                if (I == t && J == t) v += tri_at(AT, w, 0, 0, 4, AT, r, c);
                if (I == h && J == t) v += tri_at(AH, w, 0, 0, 4, AT, r, c);
            } else if (pi && j < 4) {
                if (I == h) v += row_dot(AH, r, w, 0, 0, 0, c);
                if (I == t) v += row_dot(AT, r, w, 0, 0, 0, c);
            } else if (pi) {
                if (I == h) v += row_dot(AH, r, w, 0, 0, 12, 0);
                if (I == t) v += row_dot(AT, r, w, 0, 0, 12, 0);
            } else {
                v += h13_at(w, r, j == N ? 12 : c);
            }
        }
    return v;
}
EDS_HD double top_entry(int F, const double* acc, const double* adH, const double* adT, int i, int j) {
    const int N = 4 + 8 * F;
    if (j == N) return top_raw(F, acc, adH, adT, i, j);
    if (i < 4 && j >= 4) return top_raw(F, acc, adH, adT, j, i);
    if (i >= 4 && j >= 4) {
        const int I = (i - 4) / 8, J = (j - 4) / 8;
        if (I < J) return top_raw(F, acc, adH, adT, i, j) + top_raw(F, acc, adH, adT, j, i);
        if (I > J) return top_raw(F, acc, adH, adT, j, i) + top_raw(F, acc, adH, adT, i, j);
    }
    return top_raw(F, acc, adH, adT, i, j);
}
EDS_HD double sc_entry(int F, const double* acc, const double* adH, const double* adT, int i, int j) {
    const int N = 4 + 8 * F;
    if (i < 4 && j >= 4 && j < N) { const int t = i; i = j; j = t; }          // the calibration rows are the transposed copies
    if (i < 4) {                                                                 // accHcc, accbc: hosts left to right
        const double* C = acc + acc_off_c(F);
        double v = 0.0;
        for (int h = 0; h < F; ++h) v += C[h * C_WORDS + (j == N ? 16 + i : 4 * i + j)];
        return v;
    }
    const int I = (i - 4) / 8, r = (i - 4) % 8;
    const bool pj = j >= 4 && j < N;
    const int J = pj ? (j - 4) / 8 : -1, c = pj ? (j - 4) % 8 : j;
    double v = 0.0;
    for (int a = 0; a < F; ++a)
        for (int b = 0; b < F; ++b) {
            if (I != a && I != b) continue;                      // this pair adds nothing to a row of block I
            const int ij = a + F * b;
            const double *AH = adH + 64 * ij, *AT = adT + 64 * ij;
            const double* E = acc + acc_off_e(F) + (size_t)ij * E_WORDS;
            if (!pj) {
                if (j < 4) {
                    if (I == a) v += row_dot(AH, r, E, 1, 4, 0, c);
                    if (I == b) v += row_dot(AT, r, E, 1, 4, 0, c);
                } else {
                    if (I == a) v += row_dot(AH, r, E + 32, 1, 1, 0, 0);
                    if (I == b) v += row_dot(AT, r, E + 32, 1, 1, 0, 0);
                }
                continue;
            }
            for (int k = 0; k < F; ++k) {
                const double* D = acc + acc_off_d(F) + (size_t)(ij + k * F * F) * D_WORDS;
                if (D[64] == 0.0) continue;
                const int ik = a + F * k;
                if (I == a && J == a) v += tri_at(AH, D, 1, 8, 0, adH + 64 * ik, r, c);
                if (I == b && J == k) v += tri_at(AT, D, 1, 8, 0, adT + 64 * ik, r, c);
                if (I == b && J == a) v += tri_at(AT, D, 1, 8, 0, adH + 64 * ik, r, c);
                if (I == a && J == k) v += tri_at(AH, D, 1, 8, 0, adT + 64 * ik, r, c);
            }
        }
    return v;
}
// out: H_A (N N), b_A (N), H_sc (N N), b_sc (N), one after the other; entry e of 2 N (N + 1)
EDS_HD int stitch_words(int F) { const int N = 4 + 8 * F; return 2 * N * (N + 1); }
EDS_HD void stitch_entry(int F, const double* acc, const double* adH, const double* adT, int e, double* out) {
    const int N = 4 + 8 * F, half = N * (N + 1), q = e % half;
    const int i = q < N * N ? q / N : q - N * N, j = q < N * N ? q % N : N;
    out[e] = e < half ? top_entry(F, acc, adH, adT, i, j) : sc_entry(F, acc, adH, adT, i, j);
}

}  // namespace edswin
