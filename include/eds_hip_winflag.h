/* eds_hip_winflag.h — each point's residual history kept on the device beside the eds_win of eds_hip_window.h, and the two loops of
 * DSO's FullSystem that drive it — makeKeyFrame's "every old point gets a residual towards the new keyframe", and the
 * fixLinearization == true half of linearizeAll (applyRes(true), maxRelBaseline, numGoodResiduals, lastResiduals) — and
 * flagPointsForRemoval with isOOB and isInlierNew (reference src/bundles/HessianBlocks.h:474-504), whose fates stay on the device for
 * the marginalisation and the removal that follow.  With these a keyframe cycle passes no per-point or
 * per-residual array across the bus in either direction; counts and the frame-sized matrices still cross.  FullSystem is not in
 * the reference tree, so the loops are stated here in full; the statements are the specification.  The symbols are exported by
 * libeds_hip.so; no entry point of the other headers changes its results, and a process that never calls eds_wfl_* allocates and
 * launches nothing new.
 *
 * NOT here: flagFramesForMarginalization's decision, which is a handful of comparisons over F frames and stays with the caller
 * (eds_wfl_flag_points returns the per-host totals it needs); setNewFrameEnergyTH; the connectivity map.
 *
 * THE COLUMNS.  Allocated by the first eds_wfl_* call that needs them (set_history, get_history, insert_frame_residuals, apply_fixed
 * or flag_points) for the
 * window's whole capacity, with the defaults below.
 *  - per point: num_good (int32, numGoodResiduals), max_rel_baseline (fp32, maxRelBaseline), last_target[2] (int32: the target frame
 *    of lastResiduals[k].first, -1 for a null pointer), last_state[2] (int32 ResState, lastResiduals[k].second; [0] is the latest);
 *  - per residual: is_new (int32, isNew).
 * A residual is identified by (point, target): lastResiduals[k].first == r reads last_target[k] == target(r) for a residual r of that
 * point.  Defaults (the constructors' values): num_good 0, max_rel_baseline 0, last_target -1, last_state OOB (1), is_new 1.
 *
 * Once allocated the columns travel with every eds_wed_* edit (eds_hip_winedit.h) through the same gathers as the window's rows:
 *  - a residual removed by eds_wed_remove_residuals or eds_wed_marginalize_frame sets any last_target[k] of its point that named it
 *    to -1 and keeps last_state[k] (DSO's removal loops set .first = 0);
 *  - eds_wed_marginalize_frame lowers every last_target[k] > frame by one;
 *  - eds_wed_remove_points moves the surviving points' history with them;
 *  - eds_wed_insert_activated gives a new point num_good = 0, max_rel_baseline = 0, last_target[0] = F - 1 with state IN if it got
 *    a residual towards frame F - 1, else -1 with state OOB; the same for [1] and frame F - 2; is_new = 1 on its residuals.
 * eds_win_set_points and eds_win_set_residuals put every column back to its defaults: the tables are new.
 * Before the first eds_wfl_* call none of this runs.
 *
 * Conventions are those of eds_hip_winedit.h: plain pointers, EDS_OK or a negative eds_status, eds_last_error() for the text; every
 * call returns when its results are on the device (tables) or the host (counts).  A refused call changes nothing.
 */
#ifndef EDS_HIP_WINFLAG_H_
#define EDS_HIP_WINFLAG_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip_winedit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_WINFLAG_ABI_VERSION 1
int eds_wfl_abi_version(void);

/* the columns, n points and m residuals */
typedef struct eds_wfl_history {
    int32_t* num_good;                            /* n */
    float* max_rel_baseline;                      /* n */
    int32_t* last_target;                         /* n x 2 */
    int32_t* last_state;                          /* n x 2 */
    int32_t* is_new;                              /* m */
} eds_wfl_history;

/* For start-up and tests.  Any member NULL (or hist itself): that column takes its defaults.  The arrays are host memory, or device
 * memory with on_device = 1 (checked with eds_dev_check_range over the words that will be read).  Host arrays are checked:
 * last_target in -1 .. 7 and last_state in 0 .. 2, else EDS_ERR_INVALID. */
int eds_wfl_set_history(eds_win* win, const eds_wfl_history* hist, int on_device);
/* reads the columns back into host memory; any member may be NULL */
int eds_wfl_get_history(eds_win* win, const eds_wfl_history* out);

/* makeKeyFrame's loop for keyframe `frame` (0 .. max_frames - 1).  Every point whose host is not `frame` and that has no residual
 * towards `frame` gets one, at the END of the point's run.  It is exactly what eds_win_set_residuals leaves for state IN and energy
 * 0: new state OUTLIER, not active, J zero, not linearized; is_new = 1.  For each such point last[1] = last[0], then last[0] =
 * (frame, IN).  Every other row keeps its values: the rows move through the gathers of eds_hip_winedit.h (a stable edit), and only
 * the points' flags and the count cross the bus.  The window's linearized mark is cleared (eds_win_apply is EDS_ERR_STATE until the
 * next eds_win_linearize); an eds_wsv state stays valid.  EDS_ERR_STATE beyond max_residuals, with nothing changed.
 * inserted_out (may be NULL): the residuals inserted. */
int eds_wfl_insert_frame_residuals(eds_win* win, int frame, int32_t* inserted_out);

/* The fixLinearization == true half of linearizeAll, after an eds_win_linearize (EDS_ERR_STATE without one).  F and precalc are
 * those of that eds_win_linearize (F x F records of EDS_WIN_PRECALC_FLOATS floats, [host F + target], finite).
 *  1. applyRes(true) for every residual: the results of eds_win_apply(win, 1), bit for bit (the same kernel).
 *  2. For every residual that is then active and has is_new != 0, with (u, v) and idepth_scaled its point's:
 *       ptp_inf = PRE_KRKiTll (u, v, 1), each row summed left to right as item 2 of eds_hip_window.h states;
 *       ptp = ptp_inf + PRE_KtTll * idepth_scaled;
 *       dx = ptp_inf[0] / ptp_inf[2] - ptp[0] / ptp[2], dy likewise;
 *       relBS = (float)(0.01 * (double)sqrtf(dx * dx + dy * dy));
 *       if (relBS > max_rel_baseline) max_rel_baseline = relBS (a NaN never wins); num_good += 1.
 *     One lane walks a point's run in table order: no atomic, one order.
 *  3. For every residual: last_state[k] = state where last_target[k] == target, testing [0] first, else [1].
 *  4. clear_is_new = 1 sets every is_new to 0 afterwards; with 0 the flags stay.  Upstream DSO sets isNew in the residual's
 *     constructor and, as far as the code known here goes, never clears it: 0 is that reading, 1 the one the name suggests.
 * counts (may be NULL): the residuals now IN / OOB / OUTLIER.  The caller follows with eds_wed_remove_residuals(win, NULL, ..), which
 * is DSO's toRemove loop.  EDS_ERR_INVALID: F outside 2 .. max_frames, a host or target not below F, clear_is_new neither 0 nor 1, a
 * NULL or not finite precalc. */
int eds_wfl_apply_fixed(eds_win* win, int F, const float* precalc, int clear_is_new, int32_t* counts /* [3] */);

/* the setting_* values flagPointsForRemoval reads (reference src/utils/settings.cpp:68, 106-107) */
typedef struct eds_wfl_params {
    int32_t min_good_active_res_for_marg;         /* setting_minGoodActiveResForMarg = 3 */
    int32_t min_good_res_for_marg;                /* setting_minGoodResForMarg = 4 */
    float min_idepth_h_marg;                      /* setting_minIdepthH_marg = 50 */
    int32_t reserved;
} eds_wfl_params;
void eds_wfl_params_default(eds_wfl_params* params);

#define EDS_WFL_KEEP 0
#define EDS_WFL_MARGINALIZE 1
#define EDS_WFL_DROP 2
/* flagPointsForRemoval; with only_empty = 1 removeOutliers' point loop.  frames_to_marg: bit f set where frame f is
 * flaggedForMarginalization (no bit at or above F).  F, precalc and frame_energy_th as eds_win_linearize takes them; F is the eds_wsv
 * state's.  Per point the fate is KEEP, MARGINALIZE or DROP, decided in this order:
 *  - idepth_scaled < 0 or an empty run: DROP.  With only_empty only the empty run counts and everything else is KEEP.
 *  - else, if isOOB holds or the host's bit is set in the mask:
 *      if isInlierNew holds (run length >= min_good_active_res_for_marg && num_good >= min_good_res_for_marg), then for every residual of
 *      the point, in order: resetOOB (state_NewEnergy = state_energy = 0, state_NewState = OUTLIER, state = IN; Residuals.h:92-98),
 *      linearize, isLinearized = false, applyRes(true), fixLinearizationF where the residual is then active
 *      (EnergyFunctionalStructs.cpp:87-113) — the kernels of eds_win_linearize, eds_win_apply and eds_wsv_fix_linearization behind a
 *      device mask, bit for bit what those calls give for the same residuals; then idepth_hessian > min_idepth_h_marg: MARGINALIZE,
 *      else DROP.  idepth_hessian is the value the last eds_win_point_hessians / eds_win_accumulate left, not recomputed.
 *      Else DROP.
 *  - else KEEP.
 * isOOB is literally HessianBlocks.h:474-497, the run length playing residuals.size(): visInToMarg counts the residuals of state IN
 * whose target's bit is set; then, in this order,
 *      size >= min_good_active_res_for_marg && num_good > min_good_res_for_marg + 10 && size - visInToMarg < min_good_active_res_for_marg: true;
 *      last_state[0] == OOB: true;  size < 2: false;  last_state[0] == OUTLIER && last_state[1] == OUTLIER: true;  false.
 * Phase one is one lane per point walking its run; phase two runs over the residuals of the points phase one chose.  The fates stay on
 * the device in the window; any edit of the tables and eds_win_set_points / eds_win_set_residuals make them stale.
 * counts (may be NULL): kept, marginalised, dropped, then the same three per host frame (27 words): the in / out numbers
 * flagFramesForMarginalization needs.  EDS_ERR_STATE without a valid eds_wsv state, a calibration or the F frames; EDS_ERR_INVALID
 * for an F that is not the state's, a mask bit at or above F, only_empty neither 0 nor 1, NULL or not finite inputs.  Every refusal
 * leaves everything unchanged. */
int eds_wfl_flag_points(eds_win* win, int F, uint32_t frames_to_marg, const eds_wfl_params* params, const float* precalc, const float* frame_energy_th,
                        int only_empty, int32_t* counts /* [3 + 8 * 3] */);
/* the fates of the n points, for tests; EDS_ERR_STATE when none are current */
int eds_wfl_get_fates(eds_win* win, int32_t* fate);
/* eds_wsv_marginalize_points for the points with fate MARGINALIZE: the same code with the upload of the flags skipped.  Follows
 * eds_wfl_flag_points directly (every active residual of those points is linearized by then).  EDS_ERR_STATE when no fates are
 * current. */
int eds_wfl_marginalize_flagged(eds_win* win, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m);
/* eds_wed_remove_points for the points whose fate is not KEEP.  EDS_ERR_STATE when no fates are current; they are stale afterwards. */
int eds_wfl_remove_flagged(eds_win* win, int32_t* points_gone, int32_t* residuals_gone);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_WINFLAG_H_ */
