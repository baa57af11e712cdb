// Each point's residual history kept beside the window's tables (include/eds_hip_winflag.h): what the device kernels
// (eds_winflag.hip, and the edits of eds_winedit.hip once the columns exist) and the host share — a new point's history, what a
// removed residual and a leaving frame do to it, which points get a residual towards a new keyframe and where it goes, and the
// fixLinearization half of linearizeAll per point.  Integers, copies and one fp32 expression (rel_baseline, in one stated order), so
// host and device agree bit for bit.  Plain C++ outside hipcc.
//
// A residual is (point, target): lastResiduals[k].first == r reads last_target[2 p + k] == target(r) for a residual of point p, and
// a null pointer is -1.
#pragma once
#include <cmath>
#include <cstdint>

#include "eds_dso_common.hpp"

namespace edswfl {

constexpr int ST_IN = 0, ST_OOB = 1, ST_OUTLIER = 2;            // ResState (Residuals.h:47)
constexpr int PRECALC_FLOATS = 27;                              // PRE_KRKiTll[9], PRE_KtTll[3], ... (include/eds_hip_window.h)

// the columns: per point num_good, max_rel_baseline, last_target[2], last_state[2] ([0] is the latest); per residual is_new
struct Hist {
    int32_t* num_good;
    float* max_rel_baseline;
    int32_t *last_target, *last_state, *is_new;
};

// ---- a point's and a residual's first values (PointHessian's and PointFrameResidual's constructors) -------------------------------------
EDS_HD void default_point(const Hist& h, int p) {
    h.num_good[p] = 0;
    h.max_rel_baseline[p] = 0.0f;
    h.last_target[2 * p] = h.last_target[2 * p + 1] = -1;
    h.last_state[2 * p] = h.last_state[2 * p + 1] = ST_OOB;
}
// an activated point enters a window of F frames: lastResiduals[0] is its residual towards frame F - 1 and [1] the one towards F - 2,
// where the fit gave it one (state IN); a null pointer with state OOB otherwise
EDS_HD void activated_point(const Hist& h, int q, int F, int got_last, int got_prev) {
    h.num_good[q] = 0;
    h.max_rel_baseline[q] = 0.0f;
    h.last_target[2 * q] = got_last ? F - 1 : -1;
    h.last_state[2 * q] = got_last ? ST_IN : ST_OOB;
    h.last_target[2 * q + 1] = got_prev ? F - 2 : -1;
    h.last_state[2 * q + 1] = got_prev ? ST_IN : ST_OOB;
}

// ---- the edits -----------------------------------------------------------------------------------------------------------------------------
// the residual (p, target) leaves: lastResiduals[k].first = 0 where it named that residual; the state stays
EDS_HD void forget_residual(int32_t* last_target, int p, int target) {
    for (int k = 0; k < 2; ++k)
        if (last_target[2 * p + k] == target) last_target[2 * p + k] = -1;
}
// frame `frame` left the window: the frames above it are one lower; -1 stays
EDS_HD int32_t target_after(int32_t t, int frame) { return t > frame ? t - 1 : t; }

// ---- makeKeyFrame's loop: every point not hosted by `frame` and without a residual towards it gets one, at the END of its run -------------
EDS_HD int32_t needs_residual(const int32_t* res_first, const int32_t* res_target, int host, int p, int frame) {
    if (host == frame) return 0;
    for (int r = res_first[p]; r < res_first[p + 1]; ++r)
        if (res_target[r] == frame) return 0;
    return 1;
}
// excl[p]: the new residuals of the points before p.  Old residual r of point p moves to r + excl[p]; p's new one sits behind its run
EDS_HD int moved_row(const int32_t* excl, int p, int r) { return r + excl[p]; }
EDS_HD int new_row(const int32_t* res_first, const int32_t* excl, int p) { return res_first[p + 1] + excl[p]; }
EDS_HD int32_t moved_first(const int32_t* res_first, const int32_t* excl, int q) { return res_first[q] + excl[q]; }   // q = n: the table's end
// p->lastResiduals[1] = p->lastResiduals[0]; p->lastResiduals[0] = (r, IN)
EDS_HD void shift_last(const Hist& h, int p, int frame) {
    h.last_target[2 * p + 1] = h.last_target[2 * p];
    h.last_state[2 * p + 1] = h.last_state[2 * p];
    h.last_target[2 * p] = frame;
    h.last_state[2 * p] = ST_IN;
}

// ---- the fixLinearization half of linearizeAll, after applyRes(true) ---------------------------------------------------------------------
// relBS of one residual: pc is the (host, target) precalc record; every row of PRE_KRKiTll (u, v, 1) is summed left to right
EDS_HD float rel_baseline(const float* pc, float u, float v, float idepth_scaled) {
    const float i0 = (pc[0] * u + pc[1] * v) + pc[2] * 1.0f;
    const float i1 = (pc[3] * u + pc[4] * v) + pc[5] * 1.0f;
    const float i2 = (pc[6] * u + pc[7] * v) + pc[8] * 1.0f;
    const float p0 = i0 + pc[9] * idepth_scaled, p1 = i1 + pc[10] * idepth_scaled, p2 = i2 + pc[11] * idepth_scaled;
    const float dx = i0 / i2 - p0 / p2, dy = i1 / i2 - p1 / p2;
    return (float)(0.01 * (double)sqrtf(dx * dx + dy * dy));
}
// One point, its residuals in table order.  pcs: F x F records, [host F + target].  counts[state] += 1 for every residual.
EDS_HD void apply_fixed_point(const Hist& h, int p, const int32_t* res_first, const int32_t* res_target, const int32_t* state, const int32_t* active,
                                  const float* pcs, int F, int host, float u, float v, float idepth_scaled, int clear_is_new, int32_t* counts) {
    int32_t good = h.num_good[p], t0 = h.last_target[2 * p], t1 = h.last_target[2 * p + 1], s0 = h.last_state[2 * p], s1 = h.last_state[2 * p + 1];
    float best = h.max_rel_baseline[p];
    for (int r = res_first[p]; r < res_first[p + 1]; ++r) {
        const int t = res_target[r], s = state[r];
        if (active[r] && h.is_new[r] != 0) {
            const float rel = rel_baseline(pcs + (size_t)(host * F + t) * PRECALC_FLOATS, u, v, idepth_scaled);
            if (rel > best) best = rel;                         // a NaN never wins
            ++good;
        }
        if (t0 == t) s0 = s;
        else if (t1 == t) s1 = s;
        if (s >= 0 && s <= 2) ++counts[s];
        if (clear_is_new) h.is_new[r] = 0;
    }
    h.num_good[p] = good;
    h.max_rel_baseline[p] = best;
    h.last_state[2 * p] = s0;
    h.last_state[2 * p + 1] = s1;
}

// ---- flagPointsForRemoval -------------------------------------------------------------------------------------------------------------
constexpr int KEEP = 0, MARGINALIZE = 1, DROP = 2, CANDIDATE = 3;   // CANDIDATE: between the two phases only — to be re-linearized, then 1 or 2
// setting_minGoodActiveResForMarg, setting_minGoodResForMarg, setting_minIdepthH_marg (settings.cpp:68, 106-107)
struct Params { int32_t min_good_active_res_for_marg, min_good_res_for_marg; float min_idepth_h_marg; int32_t reserved; };
EDS_HD Params params_default() { Params p = {3, 4, 50.0f, 0}; return p; }

// PointHessian::isOOB (HessianBlocks.h:474-497) with toMarg as a bit mask of frames; the run length plays residuals.size()
EDS_HD bool is_oob(const Params& s, const Hist& h, int p, const int32_t* res_first, const int32_t* res_target, const int32_t* state, uint32_t frames_to_marg) {
    const int size = res_first[p + 1] - res_first[p];
    int vis_in_to_marg = 0;
    for (int r = res_first[p]; r < res_first[p + 1]; ++r) {
        if (state[r] != ST_IN) continue;
        if (frames_to_marg >> res_target[r] & 1u) ++vis_in_to_marg;
    }
    if (size >= s.min_good_active_res_for_marg && h.num_good[p] > s.min_good_res_for_marg + 10 && size - vis_in_to_marg < s.min_good_active_res_for_marg) return true;
    if (h.last_state[2 * p] == ST_OOB) return true;
    if (size < 2) return false;
    if (h.last_state[2 * p] == ST_OUTLIER && h.last_state[2 * p + 1] == ST_OUTLIER) return true;
    return false;
}
// PointHessian::isInlierNew (HessianBlocks.h:500-504)
EDS_HD bool is_inlier_new(const Params& s, const Hist& h, int p, const int32_t* res_first) {
    return res_first[p + 1] - res_first[p] >= s.min_good_active_res_for_marg && h.num_good[p] >= s.min_good_res_for_marg;
}
// phase one: KEEP, DROP, or CANDIDATE (its residuals are re-linearized before finish_fate decides between MARGINALIZE and DROP)
EDS_HD int32_t first_fate(const Params& s, const Hist& h, int p, int host, float idepth_scaled, const int32_t* res_first, const int32_t* res_target,
                              const int32_t* state, uint32_t frames_to_marg, int only_empty) {
    const bool empty = res_first[p + 1] == res_first[p];
    if (only_empty) return empty ? DROP : KEEP;
    if (idepth_scaled < 0 || empty) return DROP;
    if (is_oob(s, h, p, res_first, res_target, state, frames_to_marg) || (frames_to_marg >> host & 1u)) return is_inlier_new(s, h, p, res_first) ? CANDIDATE : DROP;
    return KEEP;
}
// resetOOB (Residuals.h:92-98) and isLinearized = false for one residual of a candidate
EDS_HD void reset_oob(int r, int32_t* state, int32_t* new_state, float* energy, float* new_energy, int32_t* lin) {
    new_energy[r] = 0.0f; energy[r] = 0.0f;
    new_state[r] = ST_OUTLIER;
    state[r] = ST_IN;
    lin[r] = 0;
}
// phase two's end: the Hessian the last eds_win_point_hessians / eds_win_accumulate left decides
EDS_HD int32_t finish_fate(const Params& s, int32_t fate, float idepth_hessian) {
    if (fate != CANDIDATE) return fate;
    return idepth_hessian > s.min_idepth_h_marg ? MARGINALIZE : DROP;
}

}  // namespace edswfl
