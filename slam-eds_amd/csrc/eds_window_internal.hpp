// What eds_window.hip, eds_winsolve.hip, eds_winedit.hip and eds_winflag.hip share: the definition of the opaque eds_win of
// include/eds_hip_window.h, the state include/eds_hip_winsolve.h keeps beside it, the second set of buffers include/eds_hip_winedit.h
// moves the rows into, the history columns of include/eds_hip_winflag.h, and the launches of eds_window.hip and eds_winedit.hip that
// the other files queue into the window's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "eds_device_owner.hpp"
#include "eds_map_internal.hpp"
#include "eds_window.hpp"

namespace edswin {
struct Sum { double energy; int32_t counts[4]; };
}

// include/eds_hip_winsolve.h's part of a window: eds_wsv_set_state allocates it through the window's owner, eds_win_destroy deletes it
// (wsv_release) once the owner has freed the device memory
struct eds_wsv_state {
    bool valid = false;                                    // eds_win_set_points and eds_win_set_residuals clear it
    bool rows_live = false;                                // the per-point and per-residual rows belong to the tables as they stand: set with the
                                                           // state, cleared with `valid` by those two calls, KEPT when a frame leaves (eds_hip_winedit.h)
    bool lf_on_device = false;                             // eds_win::lf holds the sums modes 1 / 2 wrote
    bool have_backup = false, have_step = false, have_system = false;
    std::vector<double> last_x;                            // x of the last solve
    int F = 0;
    int32_t* lin = nullptr;                                // [max_residuals] isLinearized
    int32_t* sel = nullptr;                                // [max(max_residuals, max_points)] a call's selection
    float *rtz = nullptr, *res_approx = nullptr;           // [max_residuals][8] res_toZeroF, resApprox
    float *adF = nullptr, *adHTdeltaF = nullptr;           // adHostF then adTargetF [2][64][64]; [64][8]
    float *cF = nullptr;                                   // cDeltaF[4], cPriorF[4]
    float *xAd = nullptr, *step = nullptr, *backup = nullptr;   // [64][8] then cstep[4]; [max_points]; [max_points]
    double *ad = nullptr;                                  // adHost then adTarget as doubles [2][64][64]
    double *vec = nullptr;                                 // delta[68], prior[68], prior * delta_prior[68], delta_prior[68]
    double *accL = nullptr, *work = nullptr;               // the accumulators of mode 1; the solve's matrices (edswsv::work_words)
    double *stL = nullptr;                                 // mode 1's stitch H_L, b_L
    int32_t* flag = nullptr;                               // [4] x not finite, residuals modes 1 / 2 added, residuals that refuse a marginalisation
    double* e_out = nullptr;                               // [2] an energy
};

// include/eds_hip_winedit.h's part of a window: the first eds_wed_* call allocates it, likewise (wed_release).  An edit
// gathers every row into the second set and then exchanges the pointers with the window's (and the eds_wsv state's) own.
struct eds_wed_state {
    edswin::Point* pts = nullptr;
    float *ids = nullptr, *idz = nullptr, *prior = nullptr, *delta = nullptr, *lf = nullptr;
    edswin::PointOut* pout = nullptr;
    int32_t *res_first = nullptr, *res_point = nullptr, *res_target = nullptr, *state = nullptr, *new_state = nullptr, *active = nullptr;
    float *energy = nullptr, *new_energy = nullptr, *new_energy_wo = nullptr, *ret = nullptr, *cp = nullptr, *proj = nullptr, *J = nullptr,
          *efJ = nullptr, *JpJdF = nullptr;
    bool have_wsv = false;                                 // the second set of the eds_wsv state's rows, allocated once such a state exists
    int32_t* lin = nullptr;
    float *rtz = nullptr, *res_approx = nullptr, *step = nullptr, *backup = nullptr;
    int32_t* flag = nullptr;                               // [max(max_points, max_residuals)] the caller's flags
    int32_t *keep_r = nullptr, *excl_r = nullptr, *map_r = nullptr;   // [max_residuals], [max_residuals + 1], [max_residuals]
    int32_t *keep_p = nullptr, *excl_p = nullptr, *map_p = nullptr;   // the same per point
    int32_t *block = nullptr, *total = nullptr;            // the scan's per-workgroup sums; [4] the surviving residuals and points, the frame marginalisation's flag
    // eds_wed_insert_activated, sized for the eds_imm at its first call: C candidates, G = 8 C grid cells
    size_t ins_cap = 0;
    int32_t *ins_keep = nullptr, *ins_excl_c = nullptr, *ins_excl_g = nullptr, *ins_map_c = nullptr, *ins_map_g = nullptr;   // [C + G], [C + 1], [G + 1], [C], [G]
    int32_t *ins_tile = nullptr, *ins_first = nullptr;     // the scans' tile sums; [9] the hosts' runs before the insert
    double* marg = nullptr;                                // eds_wed_marginalize_frame: HM, bM, prior, delta_prior in; then HM', bM' out
};

// include/eds_hip_winflag.h's part of a window: the first eds_wfl_* call allocates it, likewise (wfl_release).  Both sets of every
// column: the edits of eds_winedit.hip gather them with the window's rows and exchange them with the rest.
struct eds_wfl_state {
    int32_t *num_good = nullptr, *last_target = nullptr, *last_state = nullptr, *is_new = nullptr;   // [max_points], [max_points][2] twice, [max_residuals]
    float* max_rel_baseline = nullptr;                     // [max_points]
    int32_t *num_good2 = nullptr, *last_target2 = nullptr, *last_state2 = nullptr, *is_new2 = nullptr;   // the second set
    float* max_rel_baseline2 = nullptr;
    int32_t* counts = nullptr;                             // [32] a call's counts: the residuals IN / OOB / OUTLIER; or the fates' totals, then per host
    int32_t *fate = nullptr, *mask = nullptr;              // [max_points] KEEP / MARGINALIZE / DROP; a call's selection of points
    bool fates_current = false;                            // eds_wfl_flag_points sets it, every edit of the tables and eds_win_set_* clear it
};

struct eds_win {
    edscapi::DeviceOwner own;                             // the window's buffers and both states' below
    int H = 0, W = 0, max_frames = 0, max_points = 0, max_residuals = 0;
    edswin::Params prm;
    edswin::Calib cal;
    bool calib_set = false, linearized = false;
    uint32_t frames_set = 0;                              // bit f: frame f holds an image
    int n = 0, m = 0, max_host = -1, max_target = -1;
    std::vector<int32_t> host_of, h_point, h_target;     // host copies for the checks and the (point, target) -> residual map
    int32_t *res_of = nullptr, *first = nullptr;          // [max_points * 8], [9]
    double* acc = nullptr;                                // [acc_size(8)]
    double *ad = nullptr, *stitched = nullptr;            // adHost then adTarget [2][64][64]; H_A, b_A, H_sc, b_sc [stitch_words(8)]
    edswin::Px* frames = nullptr;
    float* in_img = nullptr;
    edswin::Point* pts = nullptr;
    float *ids = nullptr, *idz = nullptr;                 // idepth_scaled, idepth_zero_scaled per point
    int32_t *res_first = nullptr, *res_point = nullptr, *res_target = nullptr, *state = nullptr, *new_state = nullptr, *active = nullptr;
    float *energy = nullptr, *new_energy = nullptr, *new_energy_wo = nullptr, *ret = nullptr, *cp = nullptr, *proj = nullptr, *J = nullptr,
          *efJ = nullptr, *JpJdF = nullptr, *th = nullptr, *prior = nullptr, *delta = nullptr, *lf = nullptr;
    edswin::Precalc* pcs = nullptr;
    edswin::Sum* sum = nullptr;
    edswin::PointOut* pout = nullptr;
    int32_t* nres = nullptr;
    eds_wsv_state* wsv = nullptr;
    eds_wed_state* wed = nullptr;
    eds_wfl_state* wfl = nullptr;
    eds_map_state* map = nullptr;                         // include/eds_hip_map.h's scratch, allocated by the first eds_map_window_* call
};

namespace edswin_internal {
// isLinearized of every residual, or NULL while no eds_wsv state holds
inline const int32_t* lin_flags(const eds_win* h) { return h->wsv && h->wsv->valid ? h->wsv->lin : nullptr; }
inline bool lf_on_device(const eds_win* h) { return h->wsv && h->wsv->valid && h->wsv->lf_on_device; }
// eds_window.hip: the (point, target) -> residual map and the hosts' runs, uploaded; EDS_ERR_INVALID as eds_win_accumulate refuses
int upload_maps(eds_win* h, int F);
// eds_window.hip, queued into h->st without a wait: the per-point prologue from the device's priorF / deltaF / lf (mode 0 or 2, sel may be
// NULL), every accumulator word into `acc`, and entries [e0, e1) of both stitches from `acc` and the device adjoints into `out`
void queue_points(eds_win* h, int mode, const int32_t* sel, int shift);
void queue_acc(eds_win* h, int F, int mode, const int32_t* sel, int has_lf, int words, double* acc);
void queue_stitch(eds_win* h, int F, const double* acc, const double* ad, int entries, double* out);
// k_win_linearize (the precalc records and thresholds are in h->pcs / h->th already) and k_win_apply over every residual, or with
// `mask` (per point, device memory) over the residuals of the points it marks
void queue_linearize(eds_win* h, int F, const int32_t* mask);
void queue_apply(eds_win* h, int copy_jacobians, const int32_t* mask);
// eds_winsolve.hip
void wsv_release(eds_win* h);
void wsv_invalidate(eds_win* h);
int wsv_set_state(eds_win* h, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior, const double* delta_prior,
                  const double* cPrior, const double* cDelta, const float* priorF, const float* deltaF, bool from_device);
// k_wsv_fix for the residuals `select` (per residual, device memory) marks; eds_wsv_marginalize_points with the flags from host memory,
// or (marg == NULL) already in the state's `sel`
void wsv_queue_fix(eds_win* h, const int32_t* select);
int wsv_marginalize_points(eds_win* h, const int32_t* marg, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m);
// eds_winedit.hip
void wed_release(eds_win* h);
// ... and what an insert of eds_winflag.hip needs of it: the second set allocated, the exclusive sums of keep[0 .. n) (excl has n + 1
// entries; the scan's tiles are the state's own), every per-residual column of the new rows 0 .. rows - 1 gathered into the second set
// (row i is row map[i], zeros where map[i] < 0), and the two sets of the per-residual columns exchanged
int wed_ensure_state(eds_win* h);
int wed_queue_scan(eds_win* h, const int32_t* keep, int n, int32_t* excl, int32_t* map, int32_t* total);
void wed_queue_residual_rows(eds_win* h, const int32_t* map, int rows);
void wed_exchange_residual_sets(eds_win* h);
// eds_winflag.hip
void wfl_release(eds_win* h);
int wfl_reset(eds_win* h);                                 // the defaults over the whole capacity: the tables were set anew
}  // namespace edswin_internal
