// DSO's immature points (include/eds_hip_immature.h): what the device kernels (eds_immature.hip) and the host share — the level-0
// gradient, both constructors and ImmaturePoint::traceOn cut into the three pieces the wavefront kernel needs (what is decided before
// the search, the energy of one search step, what follows the arg-min) — and a serial restatement (trace_serial) that the CPU tests
// compare with the numpy oracle.  fp32 in the reference's order; every translation unit that includes this is built without
// contraction into FMAs.  Plain C++ outside hipcc.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eds_dso_common.hpp"

namespace edsimm {

enum Status : int32_t { GOOD = 0, OOB = 1, OUTLIER = 2, SKIPPED = 3, BADCONDITION = 4, UNINITIALIZED = 5 };
constexpr int NUM_STATUS = 6;
constexpr int PATTERN = 8;
constexpr int MAX_STEPS = 99;

// eds_imm_params, member for member
struct Params {
    float max_pix_search, trace_stepsize;
    int32_t gn_iterations;
    float gn_threshold, extra_slack_on_th, slack_interval, min_improvement_factor;
    int32_t min_trace_test_radius;
    float huber_th, outlier_th, outlier_th_sum_component, overall_energy_th_weight;
};

struct alignas(8) Grad { float x, y; };

// one frame: the colour plane the search reads, and the gradient plane only the Gauss-Newton steps read
struct Frame {
    const float* c;
    const Grad* g;
};

// one point, 32 words: a wavefront reads it with one request
struct alignas(16) Point {
    float color[PATTERN], weights[PATTERN];
    float gradH[4];                        // row-major 2 x 2
    float energyTH, u, v, quality, idepth_min, idepth_max, last_u, last_v, last_interval, type;
    int32_t status, alive;
};

struct Pre {                               // one host's hostToFrame_* and the target it is traced on
    float KRKi[9], Kt[3], aff[2];
    int32_t target, n;
};

// staticPattern[8] (reference settings.cpp:276)
EDS_HD int pat_x(int i) { const int t[PATTERN] = {0, -1, 1, -2, 0, 2, -1, 0}; return t[i]; }
EDS_HD int pat_y(int i) { const int t[PATTERN] = {-2, -1, -1, 0, 0, 0, 1, 2}; return t[i]; }

using edsdso::finite_f;
using edsdso::nan_f;

// the sample rule of the header: the cell of a VALID sample, or false
EDS_HD bool tap_cell(float x, float y, int W, int H, int* ix, int* iy) {
    if (!(fabsf(x) <= 1048576.0f && fabsf(y) <= 1048576.0f)) return false;
    const int a = (int)x, b = (int)y;
    if (a < 0 || b < 0 || a > W - 2 || b > H - 2) return false;
    *ix = a; *iy = b;
    return true;
}

// makeImages level 0 at flat index i of an H x W colour plane
EDS_HD Grad gradient_at(const float* c, int W, int H, int i) {
    Grad g = {0.0f, 0.0f};
    if (edsdso::border_row(W, H, i)) return g;
    g.x = edsdso::half_diff(c[i + 1], c[i - 1]);
    g.y = edsdso::half_diff(c[i + W], c[i - W]);
    return g;
}

// getInterpolatedElement31; NaN for an invalid sample
EDS_HD float interp31(const float* c, int W, int H, float x, float y) {
    int ix, iy;
    if (!tap_cell(x, y, W, H, &ix, &iy)) return nan_f();
    const float* bp = c + ((size_t)iy * W + ix);
    return edsdso::mix(edsdso::bilin(x, y), bp[1 + W], bp[W], bp[1], bp[0]);
}

// getInterpolatedElement33; out[0] = NaN for an invalid sample
EDS_HD void interp33(const Frame& f, int W, int H, float x, float y, float out[3]) {
    int ix, iy;
    if (!tap_cell(x, y, W, H, &ix, &iy)) { out[0] = nan_f(); out[1] = 0.0f; out[2] = 0.0f; return; }
    const edsdso::Bilin bw = edsdso::bilin(x, y);
    const size_t o = (size_t)iy * W + ix;
    const float* bp = f.c + o;
    const Grad* gp = f.g + o;
    out[0] = edsdso::mix(bw, bp[1 + W], bp[W], bp[1], bp[0]);
    out[1] = edsdso::mix(bw, gp[1 + W].x, gp[W].x, gp[1].x, gp[0].x);
    out[2] = edsdso::mix(bw, gp[1 + W].y, gp[W].y, gp[1].y, gp[0].y);
}

// Both constructors (ImmaturePoint.cpp:27-114): has_depth selects the second.
EDS_HD void construct(Point& p, const float* c, int W, int H, const Params& s, int u, int v, float type, bool has_depth, float idepth,
                          double distance) {
    p.u = (float)u; p.v = (float)v; p.type = type;
    p.idepth_min = 0.0f; p.idepth_max = nan_f(); p.status = UNINITIALIZED;
    p.quality = 10000.0f; p.last_u = 0.0f; p.last_v = 0.0f; p.last_interval = 0.0f;
    p.gradH[0] = p.gradH[1] = p.gradH[2] = p.gradH[3] = 0.0f;
    for (int i = 0; i < PATTERN; ++i) { p.color[i] = 0.0f; p.weights[i] = 0.0f; }
    p.energyTH = nan_f(); p.alive = 0;
    for (int idx = 0; idx < PATTERN; ++idx) {
        // getInterpolatedElement33BiLin at the integer pixel (u + dx, v + dy)
        const float x = (float)((int64_t)u + pat_x(idx)), y = (float)((int64_t)v + pat_y(idx));   // 64-bit: any int is a defined input
        int ix, iy;
        if (!tap_cell(x, y, W, H, &ix, &iy)) return;
        const float* bp = c + ((size_t)iy * W + ix);
        const float tl = bp[0], tr = bp[1], bl = bp[W], br = bp[W + 1];
        const float dx = x - ix, dy = y - iy;
        const float topInt = dx * tr + (1 - dx) * tl;
        const float botInt = dx * br + (1 - dx) * bl;
        const float leftInt = dy * bl + (1 - dy) * tl;
        const float rightInt = dy * br + (1 - dy) * tr;
        const float col = dx * rightInt + (1 - dx) * leftInt, gx = rightInt - leftInt, gy = botInt - topInt;
        p.color[idx] = col;
        if (!finite_f(col)) return;
        p.gradH[0] += gx * gx; p.gradH[1] += gx * gy; p.gradH[2] += gy * gx; p.gradH[3] += gy * gy;
        p.weights[idx] = sqrtf(s.outlier_th_sum_component / (s.outlier_th_sum_component + (gx * gx + gy * gy)));
    }
    float e = PATTERN * s.outlier_th;
    e *= s.overall_energy_th_weight * s.overall_energy_th_weight;
    p.energyTH = e;
    p.alive = 1;
    if (has_depth && !(distance > 1.0)) {
        p.status = GOOD;
        p.idepth_min = (float)((double)idepth - (0.1 * distance));
        p.idepth_max = (float)((double)idepth + (0.1 * distance));
    }
}

// what traceOn knows when the discrete search starts
struct Line {
    float pr[3];
    float dist, dx, dy, errorInPixel;
    float ptx, pty;                        // the position of step 0
    float rot[PATTERN][2];
    int numSteps;
};

EDS_HD void set_oob(Point& p, int status) { p.last_u = -1.0f; p.last_v = -1.0f; p.last_interval = 0.0f; p.status = status; }
EDS_HD bool inside(float u, float v, int W, int H) { return u > 4 && v > 4 && u < W - 5 && v < H - 5; }

// traceOn up to the discrete search (:130-310).  false: the point has its result; true: L describes the search.
EDS_HD bool trace_prologue(Point& p, const Params& s, int W, int H, const Pre& m, Line& L) {
    if (p.status == OOB) return false;
    const float maxPixSearch = (W + H) * s.max_pix_search;
    const float* K = m.KRKi;
    const float* Kt = m.Kt;
    for (int i = 0; i < 3; ++i) L.pr[i] = K[3 * i] * p.u + K[3 * i + 1] * p.v + K[3 * i + 2] * 1.0f;
    float ptpMin[3];
    for (int i = 0; i < 3; ++i) ptpMin[i] = L.pr[i] + Kt[i] * p.idepth_min;
    const float uMin = ptpMin[0] / ptpMin[2], vMin = ptpMin[1] / ptpMin[2];
    if (!inside(uMin, vMin, W, H)) { set_oob(p, OOB); return false; }

    float dist, uMax, vMax;
    const bool finite_max = finite_f(p.idepth_max);
    if (finite_max) {
        float ptpMax[3];
        for (int i = 0; i < 3; ++i) ptpMax[i] = L.pr[i] + Kt[i] * p.idepth_max;
        uMax = ptpMax[0] / ptpMax[2];
        vMax = ptpMax[1] / ptpMax[2];
        if (!inside(uMax, vMax, W, H)) { set_oob(p, OOB); return false; }
        dist = (uMin - uMax) * (uMin - uMax) + (vMin - vMax) * (vMin - vMax);
        dist = sqrtf(dist);
        if (dist < s.slack_interval) {
            p.last_u = (uMax + uMin) * 0.5f; p.last_v = (vMax + vMin) * 0.5f;
            p.last_interval = dist;
            p.status = SKIPPED;
            return false;
        }
    } else {
        dist = maxPixSearch;
        float ptpMax[3];
        for (int i = 0; i < 3; ++i) ptpMax[i] = L.pr[i] + Kt[i] * 0.01f;
        uMax = ptpMax[0] / ptpMax[2];
        vMax = ptpMax[1] / ptpMax[2];
        const float dx = uMax - uMin, dy = vMax - vMin;
        const float d = 1.0f / sqrtf(dx * dx + dy * dy);
        uMax = uMin + dist * dx * d;
        vMax = vMin + dist * dy * d;
        if (!inside(uMax, vMax, W, H)) { set_oob(p, OOB); return false; }
    }
    if (!(p.idepth_min < 0 || (ptpMin[2] > 0.75f && ptpMin[2] < 1.5f))) { set_oob(p, OOB); return false; }

    float dx = s.trace_stepsize * (uMax - uMin);
    float dy = s.trace_stepsize * (vMax - vMin);
    const float* G = p.gradH;
    const float a = (dx * G[0] + dy * G[2]) * dx + (dx * G[1] + dy * G[3]) * dy;
    const float b = (dy * G[0] + (-dx) * G[2]) * dy + (dy * G[1] + (-dx) * G[3]) * (-dx);
    float errorInPixel = 0.2f + 0.2f * (a + b) / a;
    if (errorInPixel * s.min_improvement_factor > dist && finite_max) {
        p.last_u = (uMax + uMin) * 0.5f; p.last_v = (vMax + vMin) * 0.5f;
        p.last_interval = dist;
        p.status = BADCONDITION;
        return false;
    }
    if (errorInPixel > 10) errorInPixel = 10;

    dx /= dist;
    dy /= dist;
    if (dist > maxPixSearch) dist = maxPixSearch;      // uMax, vMax are not read again
    const float nf = 1.9999f + dist / s.trace_stepsize;
    int numSteps = nf < 100.0f ? (int)nf : MAX_STEPS;
    const float randShift = uMin * 1000 - floorf(uMin * 1000);
    L.ptx = uMin - randShift * dx;
    L.pty = vMin - randShift * dy;
    for (int idx = 0; idx < PATTERN; ++idx) {
        const float px = (float)pat_x(idx), py = (float)pat_y(idx);
        L.rot[idx][0] = K[0] * px + K[1] * py;
        L.rot[idx][1] = K[3] * px + K[4] * py;
    }
    if (!finite_f(dx) || !finite_f(dy)) { set_oob(p, OOB); return false; }
    if (numSteps >= 100) numSteps = MAX_STEPS;
    L.dist = dist; L.dx = dx; L.dy = dy; L.errorInPixel = errorInPixel; L.numSteps = numSteps;
    return true;
}

// the energy of one search step at (ptx, pty) (:314-326)
EDS_HD float step_energy(const Point& p, const Params& s, const float* c, int W, int H, const Pre& m, const Line& L, float ptx, float pty) {
    float energy = 0;
    for (int idx = 0; idx < PATTERN; ++idx) {
        const float hitColor = interp31(c, W, H, ptx + L.rot[idx][0], pty + L.rot[idx][1]);
        if (!finite_f(hitColor)) { energy += 1e5f; continue; }
        const float residual = hitColor - (m.aff[0] * p.color[idx] + m.aff[1]);
        const float hw = fabsf(residual) < s.huber_th ? 1 : s.huber_th / fabsf(residual);
        energy += hw * residual * residual * (2 - hw);
    }
    return energy;
}

// an energy the reference's `energy < bestEnergy` can ever accept (bestEnergy starts at 1e10)
EDS_HD bool can_be_best(float e) { return e < 1e10f; }
// step i counts for the second-best score (:346-350)
EDS_HD bool outside_radius(int i, int bestIdx, int radius) { return i < bestIdx - radius || i > bestIdx + radius; }

// traceOn after the search (:351-467): quality, the Gauss-Newton steps, the outlier test, the new interval
EDS_HD void trace_epilogue(Point& p, const Params& s, const Frame& f, int W, int H, const Pre& m, const Line& L, float bestU, float bestV,
                               float bestEnergy, float secondBest) {
    const float newQuality = secondBest / bestEnergy;
    if (newQuality < p.quality || L.numSteps > 10) p.quality = newQuality;

    const float dx = L.dx, dy = L.dy;
    float uBak = bestU, vBak = bestV, gnstepsize = 1, stepBack = 0;
    if (s.gn_iterations > 0) bestEnergy = 1e5f;
    for (int it = 0; it < s.gn_iterations; ++it) {
        float Hs = 1, b = 0, energy = 0;
        for (int idx = 0; idx < PATTERN; ++idx) {
            float hit[3];
            interp33(f, W, H, bestU + L.rot[idx][0], bestV + L.rot[idx][1], hit);
            if (!finite_f(hit[0])) { energy += 1e5f; continue; }
            const float residual = hit[0] - (m.aff[0] * p.color[idx] + m.aff[1]);
            const float dResdDist = dx * hit[1] + dy * hit[2];
            const float hw = fabsf(residual) < s.huber_th ? 1 : s.huber_th / fabsf(residual);
            Hs += hw * dResdDist * dResdDist;
            b += hw * residual * dResdDist;
            energy += p.weights[idx] * p.weights[idx] * hw * residual * residual * (2 - hw);
        }
        if (energy > bestEnergy) {
            stepBack *= 0.5f;
            bestU = uBak + stepBack * dx;
            bestV = vBak + stepBack * dy;
        } else {
            float step = -gnstepsize * b / Hs;
            if (step < -0.5f) step = -0.5f;
            else if (step > 0.5f) step = 0.5f;
            if (!finite_f(step)) step = 0;
            uBak = bestU;
            vBak = bestV;
            stepBack = step;
            bestU += step * dx;
            bestV += step * dy;
            bestEnergy = energy;
        }
        if (fabsf(stepBack) < s.gn_threshold) break;
    }

    if (!(bestEnergy < p.energyTH * s.extra_slack_on_th)) {
        const int st = p.status == OUTLIER ? OOB : OUTLIER;
        set_oob(p, st);
        return;
    }
    const float e = L.errorInPixel;
    const float* Kt = m.Kt;
    float lo, hi;
    if (dx * dx > dy * dy) {
        lo = (L.pr[2] * (bestU - e * dx) - L.pr[0]) / (Kt[0] - Kt[2] * (bestU - e * dx));
        hi = (L.pr[2] * (bestU + e * dx) - L.pr[0]) / (Kt[0] - Kt[2] * (bestU + e * dx));
    } else {
        lo = (L.pr[2] * (bestV - e * dy) - L.pr[1]) / (Kt[1] - Kt[2] * (bestV - e * dy));
        hi = (L.pr[2] * (bestV + e * dy) - L.pr[1]) / (Kt[1] - Kt[2] * (bestV + e * dy));
    }
    if (lo > hi) { const float t = lo; lo = hi; hi = t; }
    p.idepth_min = lo;
    p.idepth_max = hi;
    if (!finite_f(lo) || !finite_f(hi) || (hi < 0)) { set_oob(p, OUTLIER); return; }
    p.last_interval = 2 * e;
    p.last_u = bestU;
    p.last_v = bestV;
    p.status = GOOD;
}

// traceOn, serially: the restatement the kernels are compared with
inline void trace_serial(Point& p, const Params& s, const Frame& f, int W, int H, const Pre& m) {
    if (!p.alive) return;
    Line L;
    if (!trace_prologue(p, s, W, H, m, L)) return;
    float errors[100];
    float bestU = 0, bestV = 0, bestEnergy = 1e10f;
    int bestIdx = -1;
    float ptx = L.ptx, pty = L.pty;
    for (int i = 0; i < L.numSteps; ++i) {
        const float energy = step_energy(p, s, f.c, W, H, m, L, ptx, pty);
        errors[i] = energy;
        if (energy < bestEnergy) { bestU = ptx; bestV = pty; bestEnergy = energy; bestIdx = i; }
        ptx += L.dx;
        pty += L.dy;
    }
    float secondBest = 1e10f;
    for (int i = 0; i < L.numSteps; ++i)
        if (outside_radius(i, bestIdx, s.min_trace_test_radius) && errors[i] < secondBest) secondBest = errors[i];
    trace_epilogue(p, s, f, W, H, m, L, bestU, bestV, bestEnergy, secondBest);
}

// eds_imm_set_params' rule
inline bool params_valid(const Params& s) {
    const float fl[10] = {s.max_pix_search, s.trace_stepsize, s.gn_threshold, s.extra_slack_on_th, s.slack_interval, s.min_improvement_factor,
                          s.huber_th, s.outlier_th, s.outlier_th_sum_component, s.overall_energy_th_weight};
    for (float x : fl) if (!finite_f(x)) return false;
    if (!(s.max_pix_search > 0 && s.trace_stepsize > 0 && s.huber_th > 0 && s.outlier_th_sum_component > 0)) return false;
    return s.gn_iterations >= 0 && s.gn_iterations <= 16 && s.min_trace_test_radius >= 0 && s.min_trace_test_radius <= MAX_STEPS;
}

inline Params params_default() {
    Params s;
    s.max_pix_search = 0.027f; s.trace_stepsize = 1.0f; s.gn_iterations = 3; s.gn_threshold = 0.1f; s.extra_slack_on_th = 1.2f;
    s.slack_interval = 1.5f; s.min_improvement_factor = 2.0f; s.min_trace_test_radius = 2; s.huber_th = 9.0f; s.outlier_th = 12 * 12;
    s.outlier_th_sum_component = 50 * 50; s.overall_energy_th_weight = 1.0f;
    return s;
}

}  // namespace edsimm
