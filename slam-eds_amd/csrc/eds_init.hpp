// DSO's CoarseInitializer (include/eds_hip_init.h): what the device kernels (eds_init.hip) and the host share — the point record, the
// per-tap term of calcResAndGS with its Jacobian buffer row, doStep, applyStep, optReg, resetPoints, propagateDown / propagateUp, calcEC,
// the damped loop of trackFrame and SE3::log's translation part — written ONCE over an EVALUATOR that supplies three things: a loop over
// the points of a level (each), a loop over a level's dependency schedule, depth by depth (each_sched), and the lane-strided fp64 sums
// (reduce).  SerialEv walks the device's order on the host; eds_init.hip's evaluator is one workgroup of edsdso::LANES lanes.  fp32 per tap
// and per point in the reference's order (src/init/CoarseInitializer.cpp, lines quoted as :n), fp64 sums in the order stated at the top
// of eds_dso_common.hpp; every translation unit that includes this is built without contraction into FMAs.  Plain C++ outside hipcc.
//
// THE SUMS.  Lane t adds, in fp64 and starting from 0.0, the terms of points t, t + 512, ... in that order; a point's terms are added
// one by one (for acc9: tap 0's 45 products row by row, then tap 1's, ...; the point's addend to E after them in slot 45).  The fold and
// the left-to-right addition of the eight group totals are edsdso's.  Results are cast to float where the reference holds one.
//
// THE THREE ORDER DEPENDENCIES.  optReg (:564-585), resetPoints at the top level (:785-800) and propagateUp's += (:609-617) read what
// earlier iterations of the same loop wrote.  For the first two the level carries a schedule: depth[i] = 1 + max(depth[j] : j a
// neighbour of i, j < i), the points sorted by depth (stable).  A pass first copies what it is about to change (iR; isGood) into a
// snapshot; then the depths run one after the other, and point i reads neighbour j < i from the live column (j has a smaller depth: it
// is done) and neighbour j >= i from the snapshot (the reference has not reached j yet).  propagateUp gathers per parent over its
// children in ascending order (CSR).
//
// SE3::log's atan is edsct::atan_d, beside sincos_d / exp_d in eds_coarse.hpp (within ATAN_MAX_ULP = 2 ulps of libm).
#pragma once
#include "eds_coarse.hpp"
#include "eds_nntree.hpp"

namespace edsini {

using edsct::Geo;
using edsct::Level;
using edsdso::LANES;
using edsdso::Px;

constexpr int MAX_LEVELS = edsct::MAX_LEVELS;
constexpr int NN = 10;                            // neighbours per point
constexpr int SCHED = 12;                         // words of one schedule record
constexpr int TAPS = 8;                           // patternNum: staticPattern[8] (src/utils/settings.cpp:276)
constexpr int MAX_DECISIONS = 512;                // sum over the levels of max_iterations + 1 is at most 5 * 101
constexpr int MAX_ITERATIONS = 100;

// eds_ini_params, member for member
struct Params {
    float huber_th, outlier_th, alpha_k, alpha_w, reg_weight, coupling_weight;
    int32_t fix_affine, max_iterations[MAX_LEVELS];
    float scale_xi_rot, scale_xi_trans, scale_a, scale_b;
};

// one point (the reference's Pnt without the tables and the members it never reads): 16 words
struct alignas(16) Pnt {
    float u, v, idepth, idepth_new, iR, lastHessian, lastHessian_new, maxstep, energy[2], energy_new[2], my_type, outlierTH;
    int32_t isGood, isGood_new;
};

// eds_ini_result, member for member
struct Result {
    double T[12], aff[2];
    float latest_res[3], rescale;
    int32_t snapped, frame_id, snapped_at, ready, n_decisions, launches, waits, pad;
    int32_t iters[MAX_LEVELS], accepts[MAX_LEVELS];
    uint8_t decisions[MAX_DECISIONS];              // accept (bit 0) and level (bits 1 ..) of every iteration, in order
};

// one level's points and tables.  jb: the two Jacobian buffers, [2][cap][10]; sched / doff: the dependency schedule (nd depths, the
// points of depth d are the records sched[doff[d] .. doff[d + 1]), SCHED words each: the point's index, its ten neighbours, a pad word —
// one aligned fetch gives a step all it needs before it reads other points); coff / child: the children (points of this level) of every parent (point of
// the level above), ascending
struct Lv {
    Pnt* p;
    const int32_t *sched, *parent, *doff, *coff, *child;
    float* jb;
    int32_t n, nd, n_parents, cap;
};

// what one trackFrame hands to the next
struct Carry { double T[12], aff[2]; int32_t snapped, frame_id, snapped_at, jb_cur[MAX_LEVELS]; };

struct Frame {
    Geo g;
    Params s;
    Lv lv[MAX_LEVELS];
    const Px* ref;
    Px* nw;
    const float* img;                               // the new frame, dense H x W
    float* iR_old;
    int32_t* good_old;
    float aff_guess;                                // logf(exposure_new / exposure_first), taken on the host
    int32_t have_guess, snapped_threshold, pad;
};

struct Sys { float H[64], b[8], Hsc[64], bsc[8], res[3], pad; };
// the uniform state of one trackFrame (LDS on the device): two systems and two poses (current and tried), the increment, the sums
struct Shared { Sys sys[2]; double R[2][9], t[2][3], ab[2][2]; float inc[8]; double S[46]; };

EDS_HD Params params_default() {
    Params p = {9.0f, 144.0f, 6.25f, 22500.0f, 0.8f, 1.0f, 1, {5, 5, 10, 30, 50}, 1.0f, 1.0f, 10.0f, 1000.0f};
    return p;
}
EDS_HD bool params_valid(const Params& p) {
    const float f[10] = {p.huber_th, p.outlier_th, p.alpha_k, p.alpha_w, p.reg_weight, p.coupling_weight, p.scale_xi_rot, p.scale_xi_trans,
                         p.scale_a, p.scale_b};
    for (int i = 0; i < 10; ++i) if (!edsdso::finite_f(f[i])) return false;
    for (int i = 0; i < MAX_LEVELS; ++i) if (p.max_iterations[i] < 0 || p.max_iterations[i] > MAX_ITERATIONS) return false;
    return p.huber_th > 0.0f && p.outlier_th > 0.0f && p.scale_xi_rot > 0.0f && p.scale_xi_trans > 0.0f && p.scale_a > 0.0f &&
           p.scale_b > 0.0f && (p.fix_affine == 0 || p.fix_affine == 1);
}

// ---- refToNew.log().head<3>() (sophus/se3.hpp:560-586, so3.hpp:491-531) ---------------------------------------------------------------
// edsct keeps R, not a quaternion: the quaternion is Eigen's from a rotation matrix (trace > 0: s = sqrt(trace + 1), w = s / 2, the
// vector part the antisymmetric differences times 1 / (2 s); otherwise the branch of the largest diagonal entry).  logAndTheta's three
// cases are restated (n < 1e-10; |w| < 1e-10; 2 atan(n / w) / n), and tan(theta / 2) of V^-1 is sin / cos of edsct::sincos_d.
EDS_HD void se3_log_upsilon(const double* R, const double* t, double* ups) {
    double q[3], qw;
    const double tr = (R[0] + R[4]) + R[8];
    if (tr > 0.0) {
        double s = sqrt(tr + 1.0);
        qw = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[7] - R[5]) * s; q[1] = (R[2] - R[6]) * s; q[2] = (R[3] - R[1]) * s;
    } else {
        const int i = R[8] > (R[4] > R[0] ? R[4] : R[0]) ? 2 : R[4] > R[0] ? 1 : 0;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0);
        double qq[3] = {0.0, 0.0, 0.0};
        const double h = 0.5 * s;
        s = 0.5 / s;
        qw = (R[3 * k + j] - R[3 * j + k]) * s;
        const double vj = (R[3 * j + i] + R[3 * i + j]) * s, vk = (R[3 * k + i] + R[3 * i + k]) * s;
EDS_UNROLL
        for (int m = 0; m < 3; ++m) qq[m] = m == i ? h : m == j ? vj : vk;
        q[0] = qq[0]; q[1] = qq[1]; q[2] = qq[2];
    }
    const double sq_n = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2], n = sqrt(sq_n);
    double two;
    if (n < 1e-10) two = 2.0 / qw - 2.0 * sq_n / (qw * (qw * qw));
    else if (fabs(qw) < 1e-10) two = qw > 0.0 ? 3.14159265358979323846 / n : -3.14159265358979323846 / n;
    else two = 2.0 * edsct::atan_d(n / qw) / n;
    const double theta = two * n, ox = two * q[0], oy = two * q[1], oz = two * q[2];
    const double Om[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double c2;
    if (fabs(theta) < 1e-10) c2 = 1.0 / 12.0;
    else {
        double sh, ch;
        edsct::sincos_d(theta / 2.0, &sh, &ch);
        c2 = (1.0 - theta / (2.0 * (sh / ch))) / (theta * theta);
    }
EDS_UNROLL
    for (int i = 0; i < 3; ++i) {
        double row[3];
EDS_UNROLL
        for (int j = 0; j < 3; ++j) {
            const double o2 = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
            row[j] = ((i == j ? 1.0 : 0.0) - 0.5 * Om[3 * i + j]) + c2 * o2;
        }
        ups[i] = (row[0] * t[0] + row[1] * t[1]) + row[2] * t[2];
    }
}

// ---- setFirst: one point (:725-749) ---------------------------------------------------------------------------------------------------
// the rectangle of :718-719
EDS_HD bool in_rect(int x, int y, int w, int h) { return x >= 3 && x < w - 4 && y >= 3 && y < h - 4; }
EDS_HD Pnt make_point(int x, int y, float type, const Params& s) {
    Pnt p;
    p.u = (float)(x + 0.1); p.v = (float)(y + 0.1);
    p.idepth = 1.0f; p.idepth_new = 1.0f; p.iR = 1.0f;
    p.lastHessian = 0.0f; p.lastHessian_new = 0.0f; p.maxstep = 0.0f;
    p.energy[0] = p.energy[1] = p.energy_new[0] = p.energy_new[1] = 0.0f;
    p.my_type = type; p.outlierTH = (float)TAPS * s.outlier_th;
    p.isGood = 1; p.isGood_new = 0;
    return p;
}

// ---- calcResAndGS (:265-522) ------------------------------------------------------------------------------------------------------------
struct Warp { float RKi[9], t[3], a, b, fx, fy, cx, cy, huber, wl2, hl2; int32_t w; };

// Ki is the closed form of the inverse of an upper-triangular K in fp64 (the reference inverts the fp64 K with Eigen); cx of a level is
// the fp64 value makeK forms, not its fp32 narrowing; R Ki is summed left to right in fp64 and then narrowed, as :275 does
EDS_HD Warp make_warp(const Geo& g, int lvl, const Params& s, const double* R, const double* t, double a, double b) {
    const Level& L = g.l[lvl];
    Warp w;
    const double fx = (double)L.fx, fy = (double)L.fy;
    const double cx = lvl == 0 ? (double)L.cx : ((double)g.l[0].cx + 0.5) / (double)(1 << lvl) - 0.5;
    const double cy = lvl == 0 ? (double)L.cy : ((double)g.l[0].cy + 0.5) / (double)(1 << lvl) - 0.5;
    const double fxi = 1.0 / fx, fyi = 1.0 / fy, cxi = -cx / fx, cyi = -cy / fy;
    for (int i = 0; i < 3; ++i) {
        w.RKi[3 * i + 0] = (float)(R[3 * i] * fxi);
        w.RKi[3 * i + 1] = (float)(R[3 * i + 1] * fyi);
        w.RKi[3 * i + 2] = (float)((R[3 * i] * cxi + R[3 * i + 1] * cyi) + R[3 * i + 2]);
    }
    for (int i = 0; i < 3; ++i) w.t[i] = (float)t[i];
    w.a = (float)edsct::exp_d(a); w.b = (float)b;
    w.fx = L.fx; w.fy = L.fy; w.cx = L.cx; w.cy = L.cy;
    w.huber = s.huber_th;
    w.wl2 = (float)(L.w - 2); w.hl2 = (float)(L.h - 2);
    w.w = L.w;
    return w;
}

EDS_HD float interp_c(const Px* img, float x, float y, int w) {
    const edsdso::Bilin bw = edsdso::bilin(x, y);
    const Px* bp = img + ((size_t)bw.iy * w + bw.ix);
    return edsdso::mix(bw, bp[1 + w].c, bp[w].c, bp[1].c, bp[0].c);
}

EDS_HD int sum_index(int a, int b) { return a * 9 - a * (a - 1) / 2 + (b - a); }     // (a, b), a <= b, of the 45

// one point of the first loop (:292-428): its state, its JbBuffer_new row (before the alphaOpt terms), its 45 x 8 products and its
// addend to E (slot 45).  A tap that fails ends the point as the reference's break does: later taps change nothing.
EDS_HD void point_calc(const Warp& w, const Px* ref, const Px* nw, Pnt& p, float* jb, double* acc, float* taps = nullptr) {
    p.maxstep = 1e10f;
    if (!p.isGood) {
        acc[45] += (double)p.energy[0];
        p.energy_new[0] = p.energy[0]; p.energy_new[1] = p.energy[1];
        p.isGood_new = 0;
        return;
    }
    const int PX[TAPS] = {0, -1, 1, -2, 0, 2, -1, 0}, PY[TAPS] = {-2, -1, -1, 0, 0, 0, 1, 2};
    float J[9][TAPS] = {};
    float row[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool good = true;
    float energy = 0, pmax = 1e10f;
    const float id = p.idepth_new;
EDS_UNROLL
    for (int k = 0; k < TAPS; ++k) {
        if (!good) continue;
        const float x = p.u + PX[k], y = p.v + PY[k];
        const float pt0 = ((w.RKi[0] * x + w.RKi[1] * y) + w.RKi[2] * 1.0f) + w.t[0] * id;
        const float pt1 = ((w.RKi[3] * x + w.RKi[4] * y) + w.RKi[5] * 1.0f) + w.t[1] * id;
        const float pt2 = ((w.RKi[6] * x + w.RKi[7] * y) + w.RKi[8] * 1.0f) + w.t[2] * id;
        const float u = pt0 / pt2, v = pt1 / pt2;
        const float Ku = w.fx * u + w.cx, Kv = w.fy * v + w.cy;
        const float new_idepth = id / pt2;
        if (!(Ku > 1 && Kv > 1 && Ku < w.wl2 && Kv < w.hl2 && new_idepth > 0)) { good = false; continue; }
        const edsdso::Bilin bw = edsdso::bilin(Ku, Kv);
        const Px* bp = nw + ((size_t)bw.iy * w.w + bw.ix);
        const Px v11 = bp[1 + w.w], v01 = bp[w.w], v10 = bp[1], v00 = bp[0];
        const float h0 = edsdso::mix(bw, v11.c, v01.c, v10.c, v00.c);
        const float h1 = edsdso::mix(bw, v11.dx, v01.dx, v10.dx, v00.dx);
        const float h2 = edsdso::mix(bw, v11.dy, v01.dy, v10.dy, v00.dy);
        const float rlR = interp_c(ref, x, y, w.w);
        if (!edsdso::finite_f(rlR) || !edsdso::finite_f(h0)) { good = false; continue; }
        const float residual = h0 - w.a * rlR - w.b;
        float hw = fabsf(residual) < w.huber ? 1 : w.huber / fabsf(residual);
        if (taps) { taps[2 * k] = residual; taps[2 * k + 1] = hw; }          // the host's tests read them; the device passes none
        energy += hw * residual * residual * (2 - hw);
        const float dxdd = (w.t[0] - w.t[2] * u) / pt2, dydd = (w.t[1] - w.t[2] * v) / pt2;
        if (hw < 1) hw = sqrtf(hw);
        const float dxI = hw * h1 * w.fx, dyI = hw * h2 * w.fy;
        J[0][k] = new_idepth * dxI;
        J[1][k] = new_idepth * dyI;
        J[2][k] = -new_idepth * (u * dxI + v * dyI);
        J[3][k] = -u * v * dxI - (1 + v * v) * dyI;
        J[4][k] = (1 + u * u) * dxI + u * v * dyI;
        J[5][k] = -v * dxI + u * dyI;
        J[6][k] = -hw * w.a * rlR;
        J[7][k] = -hw * 1;
        J[8][k] = hw * residual;
        const float dd = dxI * dxdd + dyI * dydd;
        const float sx = dxdd * w.fx, sy = dydd * w.fy;
        const float maxstep = 1.0f / sqrtf(sx * sx + sy * sy);
        if (maxstep < pmax) pmax = maxstep;
EDS_UNROLL
        for (int q = 0; q < 9; ++q) row[q] += J[q][k] * dd;
        row[9] += dd * dd;
    }
    p.maxstep = pmax;
EDS_UNROLL
    for (int q = 0; q < 10; ++q) jb[q] = row[q];
    if (!good || energy > p.outlierTH * 20) {
        acc[45] += (double)p.energy[0];
        p.isGood_new = 0;
        p.energy_new[0] = p.energy[0]; p.energy_new[1] = p.energy[1];
        return;
    }
    p.isGood_new = 1;
    p.energy_new[0] = energy;
EDS_UNROLL
    for (int k = 0; k < TAPS; ++k) {
        int q = 0;
EDS_UNROLL
        for (int a = 0; a < 9; ++a)
EDS_UNROLL
            for (int b = a; b < 9; ++b) { acc[q] += (double)(J[a][k] * J[b][k]); ++q; }
    }
    acc[45] += (double)energy;
}

// one point of the third loop (:474-496), with the second loop's energy_new[1] (:450): the alphaOpt and coupling terms of the row,
// 1 / (1 + x), and the 45 weighted products of updateSingleWeighted ((Ja Ja) w on the diagonal, Jb (Ja w) beside it)
EDS_HD void point_sc(Pnt& p, float* r, float alphaOpt, float coupling, double* acc) {
    if (!p.isGood_new) return;
    p.energy_new[1] = (p.idepth_new - 1) * (p.idepth_new - 1);
    p.lastHessian_new = r[9];
    r[8] += alphaOpt * (p.idepth_new - 1);
    r[9] += alphaOpt;
    if (alphaOpt == 0) {
        r[8] += coupling * (p.idepth_new - p.iR);
        r[9] += coupling;
    }
    r[9] = 1 / (1 + r[9]);
    float J[9];
EDS_UNROLL
    for (int a = 0; a < 9; ++a) J[a] = r[a];
    const float wgt = r[9];
    int q = 0;
EDS_UNROLL
    for (int a = 0; a < 9; ++a) {
        acc[q] += (double)(J[a] * J[a] * wgt); ++q;
        const float jw = J[a] * wgt;
EDS_UNROLL
        for (int b = a + 1; b < 9; ++b) { acc[q] += (double)(J[b] * jw); ++q; }
    }
}

// the whole of calcResAndGS at pose `which` into sys[which]; jb: the level's JbBuffer_new
template <class Ev>
EDS_HD void calc(Ev& ev, const Frame& f, Shared* sh, int lvl, int which, float* jb) {
    const Lv& L = f.lv[lvl];
    const int n = L.n;
    const Px *ref = f.ref + f.g.l[lvl].off, *nw = f.nw + f.g.l[lvl].off;
    const Warp w = make_warp(f.g, lvl, f.s, sh->R[which], sh->t[which], sh->ab[which][0], sh->ab[which][1]);
    ev.template reduce<46>(n, sh->S, [&](int i, double* acc) { point_calc(w, ref, nw, L.p[i], jb + (size_t)i * 10, acc); });
    Sys& y = sh->sys[which];
    const double* tt = sh->t[which];
    const double tsq = (tt[0] * tt[0] + tt[1] * tt[1]) + tt[2] * tt[2];
    float alphaEnergy = (float)((double)f.s.alpha_w * (0.0 + tsq * (double)n));          // EAlpha.A stays 0 (:439-455)
    float alphaOpt;
    if (alphaEnergy > f.s.alpha_k * n) { alphaOpt = 0; alphaEnergy = f.s.alpha_k * n; }
    else alphaOpt = f.s.alpha_w;
    if (ev.writer()) {
        for (int r = 0; r < 8; ++r) {
            for (int c = 0; c < 8; ++c) y.H[8 * r + c] = (float)sh->S[r < c ? sum_index(r, c) : sum_index(c, r)];
            y.b[r] = (float)sh->S[sum_index(r, 8)];
        }
        y.res[0] = (float)sh->S[45]; y.res[1] = alphaEnergy; y.res[2] = (float)(2 * n);  // E.num counts both loops' updates
        y.pad = 0.0f;
    }
    const float coupling = f.s.coupling_weight;
    ev.template reduce<45>(n, sh->S, [&](int i, double* acc) { point_sc(L.p[i], jb + (size_t)i * 10, alphaOpt, coupling, acc); });
    if (ev.writer()) {
        for (int r = 0; r < 8; ++r) {
            for (int c = 0; c < 8; ++c) y.Hsc[8 * r + c] = (float)sh->S[r < c ? sum_index(r, c) : sum_index(c, r)];
            y.bsc[r] = (float)sh->S[sum_index(r, 8)];
        }
        double ups[3];
        se3_log_upsilon(sh->R[which], tt, ups);
        for (int i = 0; i < 3; ++i) {
            y.H[9 * i] += alphaOpt * n;
            y.b[i] += (float)ups[i] * alphaOpt * n;
        }
    }
    ev.sync();
}

// ---- calcEC (:531-551): old and new coupling energy and the number of terms, into out[3] -------------------------------------------------
template <class Ev>
EDS_HD void calc_ec(Ev& ev, const Frame& f, Shared* sh, int lvl, int snapped, float* out) {
    const Lv& L = f.lv[lvl];
    if (!snapped) { out[0] = 0; out[1] = 0; out[2] = (float)L.n; return; }
    ev.template reduce<3>(L.n, sh->S, [&](int i, double* acc) {
        const Pnt& p = L.p[i];
        if (!p.isGood_new) return;
        const float rOld = p.idepth - p.iR, rNew = p.idepth_new - p.iR;
        acc[0] += (double)(rOld * rOld); acc[1] += (double)(rNew * rNew); acc[2] += 1.0;
    });
    out[0] = f.s.coupling_weight * (float)sh->S[0]; out[1] = f.s.coupling_weight * (float)sh->S[1]; out[2] = (float)sh->S[2];
}

// ---- optReg (:552-587) -------------------------------------------------------------------------------------------------------------------
// the nnn / 2-th smallest of v[0 .. nnn) by counting ranks: no array is permuted and every index is a constant
EDS_HD float nth_smallest(const float* v, int nnn, int k) {
    float r = 0.0f;
EDS_UNROLL
    for (int a = 0; a < NN; ++a) {
        int rank = 0;
EDS_UNROLL
        for (int b = 0; b < NN; ++b) rank += (b < nnn && (v[b] < v[a] || (v[b] == v[a] && b < a))) ? 1 : 0;
        if (a < nnn && rank == k) r = v[a];
    }
    return r;
}

template <class Ev>
EDS_HD void opt_reg(Ev& ev, const Frame& f, int lvl, int snapped) {
    const Lv& L = f.lv[lvl];
    if (!snapped) {
        ev.each(L.n, [&](int i) { L.p[i].iR = 1; });
        return;
    }
    float* old = f.iR_old;
    const float rw = f.s.reg_weight;
    ev.each(L.n, [&](int i) { old[i] = L.p[i].iR; });
    // every load of a step is issued before the first use (a -1 entry reads the point itself): one trip to memory, not ten in a chain
    ev.each_sched(L.sched, L.doff, L.nd, [&](int i, const int32_t* row) {
        Pnt& p = L.p[i];
        int32_t good[NN];
        float live[NN], snap[NN];
EDS_UNROLL
        for (int j = 0; j < NN; ++j) {
            const int o = row[j] < 0 ? i : row[j];
            good[j] = L.p[o].isGood; live[j] = L.p[o].iR; snap[j] = old[o];
        }
        if (!p.isGood) return;
        float idnn[NN] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int nnn = 0;
EDS_UNROLL
        for (int j = 0; j < NN; ++j) {
            if (row[j] == -1 || !good[j]) continue;
            const float val = row[j] < i ? live[j] : snap[j];
EDS_UNROLL
            for (int q = 0; q < NN; ++q) if (q == nnn) idnn[q] = val;
            ++nnn;
        }
        if (nnn > 2) p.iR = (1 - rw) * p.idepth + rw * nth_smallest(idnn, nnn, nnn / 2);
    });
}

// ---- resetPoints (:775-802) --------------------------------------------------------------------------------------------------------------
template <class Ev>
EDS_HD void reset_points(Ev& ev, const Frame& f, int lvl) {
    const Lv& L = f.lv[lvl];
    float* old = f.iR_old;
    int32_t* gold = f.good_old;
    ev.each(L.n, [&](int i) {
        Pnt& p = L.p[i];
        p.energy[0] = p.energy[1] = 0.0f;
        p.idepth_new = p.idepth;
        old[i] = p.iR; gold[i] = p.isGood;
    });
    if (lvl != f.g.levels - 1) return;
    ev.each_sched(L.sched, L.doff, L.nd, [&](int i, const int32_t* row) {
        Pnt& p = L.p[i];
        int32_t good[NN];
        float val[NN];
EDS_UNROLL
        for (int j = 0; j < NN; ++j) {
            const int o = row[j] < 0 ? i : row[j];
            const int32_t gl = L.p[o].isGood, gs = gold[o];
            const float vl = L.p[o].iR, vs = old[o];
            good[j] = o < i ? gl : gs; val[j] = o < i ? vl : vs;
        }
        if (p.isGood) return;
        float snd = 0, sn = 0;
EDS_UNROLL
        for (int j = 0; j < NN; ++j) {
            if (row[j] == -1 || !good[j]) continue;
            snd += val[j];
            sn += 1;
        }
        if (sn > 0) {
            p.isGood = 1;
            p.iR = p.idepth = p.idepth_new = snd / sn;
        }
    });
}

// ---- propagateDown (:632-660), propagateUp (:591-630) --------------------------------------------------------------------------------------
template <class Ev>
EDS_HD void propagate_down(Ev& ev, const Frame& f, int src, int snapped) {
    const Lv &S = f.lv[src], &T = f.lv[src - 1];
    ev.each(T.n, [&](int i) {
        Pnt& p = T.p[i];
        const Pnt& par = S.p[T.parent[i]];
        if (!par.isGood || (double)par.lastHessian < 0.1) return;
        if (!p.isGood) {
            p.iR = p.idepth = p.idepth_new = par.iR;
            p.isGood = 1;
            p.lastHessian = 0;
        } else {
            const float newiR = (p.iR * p.lastHessian * 2 + par.iR * par.lastHessian) / (p.lastHessian * 2 + par.lastHessian);
            p.iR = p.idepth = p.idepth_new = newiR;
        }
    });
    opt_reg(ev, f, src - 1, snapped);
}

template <class Ev>
EDS_HD void propagate_up(Ev& ev, const Frame& f, int src, int snapped) {
    const Lv &S = f.lv[src], &T = f.lv[src + 1];
    ev.each(T.n, [&](int i) {
        Pnt& par = T.p[i];
        float iR = 0, num = 0;
        for (int k = S.coff[i]; k < S.coff[i + 1]; ++k) {
            const Pnt& c = S.p[S.child[k]];
            if (!c.isGood) continue;
            iR += c.iR * c.lastHessian;
            num += c.lastHessian;
        }
        par.iR = iR;
        if (num > 0) {
            par.idepth = par.iR = iR / num;
            par.isGood = 1;
        }
    });
    opt_reg(ev, f, src + 1, snapped);
}

// ---- doStep (:804-832), applyStep (:834-851) ---------------------------------------------------------------------------------------------
// the dot product of :816 is summed left to right
template <class Ev>
EDS_HD void do_step(Ev& ev, const Frame& f, int lvl, float lambda, const float* inc, const float* jb) {
    const Lv& L = f.lv[lvl];
    ev.each(L.n, [&](int i) {
        Pnt& p = L.p[i];
        if (!p.isGood) return;
        const float* r = jb + (size_t)i * 10;
        float dot = r[0] * inc[0];
EDS_UNROLL
        for (int q = 1; q < 8; ++q) dot += r[q] * inc[q];
        const float b = r[8] + dot;
        float step = -b * r[9] / (1 + lambda);
        float maxstep = 0.25f * p.maxstep;
        if (maxstep > 1e10f) maxstep = 1e10f;
        if (step > maxstep) step = maxstep;
        if (step < -maxstep) step = -maxstep;
        float newIdepth = p.idepth + step;
        if ((double)newIdepth < 1e-3) newIdepth = (float)1e-3;
        if (newIdepth > 50) newIdepth = 50;
        p.idepth_new = newIdepth;
    });
}

template <class Ev>
EDS_HD void apply_step(Ev& ev, const Frame& f, int lvl) {
    const Lv& L = f.lv[lvl];
    ev.each(L.n, [&](int i) {
        Pnt& p = L.p[i];
        if (!p.isGood) { p.idepth = p.idepth_new = p.iR; return; }
        p.energy[0] = p.energy_new[0]; p.energy[1] = p.energy_new[1];
        p.isGood = p.isGood_new;
        p.idepth = p.idepth_new;
        p.lastHessian = p.lastHessian_new;
    });
}

// ---- a frame's pyramid (edsdso's level_pixel and gradient_at) -----------------------------------------------------------------------------------
template <class Ev>
EDS_HD void build_pyramid(Ev& ev, const Geo& g, const float* img, Px* px) {
    for (int l = 0; l < g.levels; ++l) {
        const Level L = g.l[l];
        Px* p = px + L.off;
        const Px* lm = l ? px + g.l[l - 1].off : nullptr;
        const int wlm1 = l ? g.l[l - 1].w : 0;
        ev.each(L.w * L.h, [&](int i) { p[i] = edsdso::level_pixel(img, lm, wlm1, L.w, i); });
        ev.each(L.w * L.h, [&](int i) {
            float dx, dy;
            edsdso::gradient_at(p, L.w, L.h, i, &dx, &dy);
            p[i].dx = dx; p[i].dy = dy;
        });
    }
}

// ---- the damped system and its solve (:148-164) ----------------------------------------------------------------------------------------------
// fp32 in the reference's order up to Hl and bl; the solve is edsct's unpivoted fp64 L D L^T of the widened system, its solution narrowed
// to float before wM multiplies it (the reference: Eigen's pivoted fp32 ldlt)
EDS_HD void solve_inc(const Sys& y, const Params& s, float lambda, int wh, float* inc) {
    const float wM[8] = {s.scale_xi_rot, s.scale_xi_rot, s.scale_xi_rot, s.scale_xi_trans, s.scale_xi_trans, s.scale_xi_trans, s.scale_a, s.scale_b};
    const float k = 1 / (1 + lambda), sc = 0.01f / wh;
    double A[64], bb[8], x[8];
    for (int r = 0; r < 8; ++r) {
        for (int c = 0; c < 8; ++c) {
            float h = y.H[8 * r + c];
            if (r == c) h *= (1 + lambda);
            h -= y.Hsc[8 * r + c] * k;
            A[8 * r + c] = (double)(wM[r] * h * wM[c] * sc);
        }
        bb[r] = (double)(wM[r] * (y.b[r] - y.bsc[r] * k) * sc);
        x[r] = 0.0;
    }
    if (s.fix_affine) edsct::ldlt_solve<6, false>(A, bb, 1.0, x);
    else edsct::ldlt_solve<8, false>(A, bb, 1.0, x);
    for (int i = 0; i < 8; ++i) inc[i] = (s.fix_affine && i >= 6) ? 0.0f : wM[i] * (float)x[i];
}

// ---- trackFrame (:75-262) --------------------------------------------------------------------------------------------------------------------
// Every caller of one evaluator runs this on the same values; the writer (lane 0, or the host) alone stores the uniform state.
template <class Ev>
EDS_HD void track_frame(Ev& ev, const Frame& f, Shared* sh, Carry* carry, Result* out) {
    const Params& s = f.s;
    const int levels = f.g.levels;
    int snapped = carry->snapped, frame_id = carry->frame_id, snapped_at = carry->snapped_at;
    unsigned jbm = 0;                                            // bit l: which of level l's two buffers is JbBuffer
    for (int l = 0; l < levels; ++l) jbm |= (unsigned)(carry->jb_cur[l] & 1) << l;
    build_pyramid(ev, f.g, f.img, f.nw);
    if (ev.writer()) {
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) sh->R[0][3 * i + j] = carry->T[4 * i + j];
            sh->t[0][i] = snapped ? carry->T[4 * i + 3] : 0.0;
        }
        sh->ab[0][0] = f.have_guess ? (double)f.aff_guess : carry->aff[0];
        sh->ab[0][1] = f.have_guess ? 0.0 : carry->aff[1];
    }
    ev.sync();
    if (!snapped)
        for (int l = 0; l < levels; ++l) {
            const Lv& L = f.lv[l];
            ev.each(L.n, [&](int i) { L.p[i].iR = 1; L.p[i].idepth_new = 1; L.p[i].lastHessian = 0; });
        }
    int cur = 0, nd = 0;
    float latest[3] = {0, 0, 0};
    for (int lvl = levels - 1; lvl >= 0; --lvl) {
        const Lv& L = f.lv[lvl];
        const int wh = f.g.l[lvl].w * f.g.l[lvl].h;
        if (lvl < levels - 1) propagate_down(ev, f, lvl + 1, snapped);
        reset_points(ev, f, lvl);
        calc(ev, f, sh, lvl, cur, L.jb + (size_t)(1 - ((jbm >> lvl) & 1)) * L.cap * 10);
        float res_old[3] = {sh->sys[cur].res[0], sh->sys[cur].res[1], sh->sys[cur].res[2]};
        apply_step(ev, f, lvl);
        jbm ^= 1u << lvl;
        float lambda = (float)0.1;
        const float eps = 1e-4f;
        int fails = 0, iteration = 0, its = 0, acc = 0;
        while (true) {
            const int nxt = 1 - cur;
            if (ev.writer()) {
                float inc[8];
                double xi[6];
                solve_inc(sh->sys[cur], s, lambda, wh, inc);
                for (int i = 0; i < 8; ++i) sh->inc[i] = inc[i];
                for (int i = 0; i < 6; ++i) xi[i] = (double)inc[i];
                edsct::se3_exp_mul(xi, sh->R[cur], sh->t[cur], sh->R[nxt], sh->t[nxt]);
                sh->ab[nxt][0] = sh->ab[cur][0] + (double)inc[6];
                sh->ab[nxt][1] = sh->ab[cur][1] + (double)inc[7];
            }
            ev.sync();
            float inc[8];
EDS_UNROLL
            for (int i = 0; i < 8; ++i) inc[i] = sh->inc[i];
            do_step(ev, f, lvl, lambda, inc, L.jb + (size_t)((jbm >> lvl) & 1) * L.cap * 10);
            calc(ev, f, sh, lvl, nxt, L.jb + (size_t)(1 - ((jbm >> lvl) & 1)) * L.cap * 10);
            float reg[3];
            calc_ec(ev, f, sh, lvl, snapped, reg);
            const float res_new[3] = {sh->sys[nxt].res[0], sh->sys[nxt].res[1], sh->sys[nxt].res[2]};
            const float eTotalNew = res_new[0] + res_new[1] + reg[1];
            const float eTotalOld = res_old[0] + res_old[1] + reg[0];
            const bool accept = eTotalOld > eTotalNew;
            if (ev.writer() && nd < MAX_DECISIONS) out->decisions[nd] = (uint8_t)((accept ? 1 : 0) | (lvl << 1));
            ++nd; ++its;
            if (accept) {
                if (res_new[1] == s.alpha_k * L.n) snapped = 1;
                cur = nxt;
                res_old[0] = res_new[0]; res_old[1] = res_new[1]; res_old[2] = res_new[2];
                apply_step(ev, f, lvl);
                jbm ^= 1u << lvl;
                opt_reg(ev, f, lvl, snapped);
                lambda = (float)(lambda * 0.5);
                fails = 0;
                if ((double)lambda < 0.0001) lambda = (float)0.0001;
                ++acc;
            } else {
                fails++;
                lambda *= 4;
                if (lambda > 10000) lambda = 10000;
            }
            float nrm = 0;
EDS_UNROLL
            for (int i = 0; i < 8; ++i) nrm += inc[i] * inc[i];
            nrm = sqrtf(nrm);
            if (!(nrm > eps) || iteration >= s.max_iterations[lvl] || fails >= 2) break;
            iteration++;
        }
        latest[0] = res_old[0]; latest[1] = res_old[1]; latest[2] = res_old[2];
        if (ev.writer()) { out->iters[lvl] = its; out->accepts[lvl] = acc; }
    }
    for (int i = 0; i < levels - 1; ++i) propagate_up(ev, f, i, snapped);
    frame_id++;
    if (!snapped) snapped_at = 0;
    if (snapped && snapped_at == 0) snapped_at = frame_id;
    if (ev.writer()) {
        const double* R = sh->R[cur];
        const double* t = sh->t[cur];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) carry->T[4 * i + j] = out->T[4 * i + j] = R[3 * i + j];
            carry->T[4 * i + 3] = out->T[4 * i + 3] = t[i];
        }
        carry->aff[0] = out->aff[0] = sh->ab[cur][0];
        carry->aff[1] = out->aff[1] = sh->ab[cur][1];
        carry->snapped = snapped; carry->frame_id = frame_id; carry->snapped_at = snapped_at;
        for (int l = 0; l < MAX_LEVELS; ++l) carry->jb_cur[l] = (int32_t)((jbm >> l) & 1);
        for (int i = 0; i < 3; ++i) out->latest_res[i] = latest[i];
        out->rescale = (float)(1.0 * sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]));
        out->snapped = snapped; out->frame_id = frame_id; out->snapped_at = snapped_at;
        out->ready = (snapped && frame_id > snapped_at + f.snapped_threshold) ? 1 : 0;
        out->n_decisions = nd < MAX_DECISIONS ? nd : MAX_DECISIONS;
        for (int l = levels; l < MAX_LEVELS; ++l) { out->iters[l] = 0; out->accepts[l] = 0; }
    }
    ev.sync();
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------
// the tables' checks and what eds_ini_set_neighbours derives: false when an index is out of range.  sched / doff: the schedule
// of this level (doff has n + 1 entries at the most, nd + 1 are used); coff / child: the CSR of this level's points under the n_parents
// points of the level above (parent == NULL at the top level: no CSR)
inline bool derive_tables(int n, const int32_t* nb, const int32_t* parent, int n_parents, int32_t* sched, int32_t* doff, int32_t* nd_out,
                          int32_t* coff, int32_t* child) {
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < NN; ++j) if (nb[(size_t)i * NN + j] < -1 || nb[(size_t)i * NN + j] >= n) return false;
        if (parent && (parent[i] < 0 || parent[i] >= n_parents)) return false;
    }
    int32_t* depth = new int32_t[(size_t)n + 1];
    int nd = 0;
    for (int i = 0; i < n; ++i) {
        int d = 0;
        for (int j = 0; j < NN; ++j) {
            const int o = nb[(size_t)i * NN + j];
            if (o >= 0 && o < i && depth[o] + 1 > d) d = depth[o] + 1;
        }
        depth[i] = d;
        if (d + 1 > nd) nd = d + 1;
    }
    for (int d = 0; d <= nd; ++d) doff[d] = 0;
    for (int i = 0; i < n; ++i) doff[depth[i] + 1]++;
    for (int d = 0; d < nd; ++d) doff[d + 1] += doff[d];
    int32_t* fill = new int32_t[(size_t)nd + 1];
    for (int d = 0; d < nd; ++d) fill[d] = doff[d];
    for (int i = 0; i < n; ++i) {
        int32_t* rec = sched + (size_t)SCHED * fill[depth[i]]++;
        rec[0] = i;
        for (int j = 0; j < NN; ++j) rec[1 + j] = nb[(size_t)i * NN + j];
        rec[SCHED - 1] = 0;
    }
    *nd_out = nd;
    delete[] depth;
    delete[] fill;
    if (parent) {
        for (int k = 0; k <= n_parents; ++k) coff[k] = 0;
        for (int i = 0; i < n; ++i) coff[parent[i] + 1]++;
        for (int k = 0; k < n_parents; ++k) coff[k + 1] += coff[k];
        int32_t* at = new int32_t[(size_t)n_parents + 1];
        for (int k = 0; k < n_parents; ++k) at[k] = coff[k];
        for (int i = 0; i < n; ++i) child[at[parent[i]]++] = i;
        delete[] at;
    }
    return true;
}

// makeNN (:884-958) by exhaustive search — NOT the reference's tables where distances tie, kept for the tests that show the difference:
// the 10 nearest points of the level (the point itself among them) and, with `up`, the nearest point of the level above to 0.5 pt -
// 0.25.  Squared distances are fp32 as FLANNPointcloud::kdtree_distance forms them; ties go to the lower index.  Fewer than 10
// points: -1 fills.
inline void make_nn_exhaustive(int n, const float* uv, int n_up, const float* uv_up, int32_t* nb, int32_t* parent) {
    for (int i = 0; i < n; ++i) {
        float bd[NN];
        int32_t bi[NN];
        int cnt = 0;
        for (int j = 0; j < n; ++j) {
            const float d0 = uv[2 * i] - uv[2 * j], d1 = uv[2 * i + 1] - uv[2 * j + 1], d = d0 * d0 + d1 * d1;
            if (cnt == NN && !(d < bd[NN - 1])) continue;
            int at = cnt < NN ? cnt++ : NN - 1;
            while (at > 0 && d < bd[at - 1]) { bd[at] = bd[at - 1]; bi[at] = bi[at - 1]; --at; }
            bd[at] = d; bi[at] = j;
        }
        for (int k = 0; k < NN; ++k) nb[(size_t)i * NN + k] = k < cnt ? bi[k] : -1;
        if (parent && n_up > 0) {
            const float qx = uv[2 * i] * 0.5f - 0.25f, qy = uv[2 * i + 1] * 0.5f - 0.25f;
            int best = 0;
            float bestd = 0;
            for (int j = 0; j < n_up; ++j) {
                const float d0 = qx - uv_up[2 * j], d1 = qy - uv_up[2 * j + 1], d = d0 * d0 + d1 * d1;
                if (j == 0 || d < bestd) { bestd = d; best = j; }
            }
            parent[i] = best;
        }
    }
}

// makeNN (:884-958) with the reference's tables, ties included: nanoflann's build and walk as csrc/eds_nntree.hpp restates them.  Per
// point the ten neighbours in nanoflann's order (the point itself among them; fewer than 10 points: -1 fills) and, with `parent`, the
// one nearest point of the level above to 0.5f pt - 0.25f.  A tree deeper than `stack` (at most edsnn::STACK) is walked by recursion.
// Coordinates are finite and n_up >= 1 with `parent` (eds_ini_make_nn refuses anything else); a parent search that finds no point —
// every squared distance overflows — answers 0.  nb_dist (n x 10) / parent_dist (n), for tests: the squared distances, 0 where no
// index was written.
inline void make_nn(int n, const float* uv, int n_up, const float* uv_up, int32_t* nb, int32_t* parent, int stack = edsnn::STACK,
                    float* nb_dist = nullptr, float* parent_dist = nullptr, int* depth_out = nullptr) {
    edsnn::Tree t, tu;
    edsnn::build(uv, n, t);
    if (parent) edsnn::build(uv_up, n_up, tu);
    if (depth_out) { depth_out[0] = t.depth; depth_out[1] = tu.depth; }
    for (int i = 0; i < n; ++i) {
        float d[NN];
        edsnn::knn_host<NN>(t, uv, uv[2 * i], uv[2 * i + 1], nb + (size_t)i * NN, d, stack);
        for (int k = 0; nb_dist && k < NN; ++k) nb_dist[(size_t)i * NN + k] = d[k];
        if (parent) {
            int32_t pi;
            float pd;
            edsnn::knn_host<1>(tu, uv_up, uv[2 * i] * 0.5f - 0.25f, uv[2 * i + 1] * 0.5f - 0.25f, &pi, &pd, stack);
            parent[i] = pi < 0 ? 0 : pi;
            if (parent_dist) parent_dist[i] = pd;
        }
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the evaluator on the host: one thread walks the device's order
struct SerialEv {
    bool writer() const { return true; }
    void sync() {}
    template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    template <class F> void each_sched(const int32_t* sched, const int32_t* doff, int nd, F f) {
        for (int d = 0; d < nd; ++d)
            for (int k = doff[d]; k < doff[d + 1]; ++k) f(sched[(size_t)SCHED * k], sched + (size_t)SCHED * k + 1);
    }
    template <int NQ, class F> void reduce(int n, double* S, F f) {
        static thread_local double part[46][LANES];
        for (int q = 0; q < NQ; ++q) memset(part[q], 0, sizeof(part[q]));
        for (int i = 0; i < n; ++i) {
            double acc[NQ];
            for (int q = 0; q < NQ; ++q) acc[q] = part[q][i % LANES];
            f(i, acc);
            for (int q = 0; q < NQ; ++q) part[q][i % LANES] = acc[q];
        }
        for (int q = 0; q < NQ; ++q) S[q] = edsdso::reduce_lanes(part[q]);
    }
};
#endif

}  // namespace edsini
