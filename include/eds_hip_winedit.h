/* eds_hip_winedit.h — the window's tables edited on the device, over the eds_win of eds_hip_window.h and the state eds_hip_winsolve.h
 * keeps beside it: EnergyFunctional::dropResidual for a selection of residuals, dropPointsF and the removePoint half of
 * marginalizePointsF for a selection of points (reference src/bundles/EnergyFunctional.cpp:477-497, 678-716), marginalizeFrame whole
 * (:498-610) together with taking the frame out of the window, insertResidual (:417-427) / insertPoint (:462-474) for the points an eds_imm's
 * activation chose, the makeIDX bookkeeping (:914-934) that follows them, and setDeltaF's per-point line (:190) from the inverse
 * depths the device holds.  After eds_wsv_marginalize_points, after an outlier removal and when
 * a frame leaves, the caller no longer reads every row back, reshapes it and uploads it through eds_win_set_points /
 * eds_win_set_residuals (which zero every J and clear every linearized flag): the rows stay where they are, and only flags, HM / bM and
 * counts cross the bus.  The symbols are exported by libeds_hip.so; no entry point of
 * the other headers changes, and a process that never calls eds_wed_* allocates and launches nothing new.
 *
 * NOT here: SOLVER_ORTHOGONALIZE_POINTMARG / _FULL; the connectivity map.  The flags are inputs here; eds_hip_winflag.h decides them on
 * the device (flagPointsForRemoval, isOOB, isInlierNew) from a per-point history that travels with every edit of this header.
 *
 * THE ONE ORDER.  eds_hip_window.h wants the points grouped by host in nondecreasing host index and the residuals grouped by point.
 * Every edit here is STABLE: the survivors keep their relative order.  The reference's swap-with-back (removePoint and dropResidual move
 * the last element into the hole) is deliberately NOT restated: it would break the grouping, and nothing downstream depends on the
 * reference's order.  After an edit the window is, bit for bit, what its rows were before, gathered by the surviving indices:
 *  - per residual: point (renumbered), target, state / energy, new_state / new_energy / new_energy_with_outlier, the linearize return,
 *    is_active, center_projected_to, projected_to, J, ef_J, JpJdF; where an eds_wsv state was ever set also is_linearized, res_toZeroF
 *    and resApprox;
 *  - per point: host, uv, color, weights, idepth_scaled, idepth_zero_scaled, the eds_win_point_out fields, priorF, deltaF, the six L
 *    sums; where an eds_wsv state was ever set also step and the idepth backup.
 * The rows move OUT OF PLACE into a second set of buffers, allocated at the first eds_wed_* call, which then changes places with the
 * first; the surviving indices come from an integer prefix sum on the device (one pass of per-workgroup sums, one workgroup that
 * scans them, one pass that scatters); J and ef_J (74 words a row) move in 16-byte pieces, 19 lanes a row, the other columns a word a
 * lane.  The window's host copies (point, target and host per row, the counts, the largest host and target) follow the same flags,
 * read back from the device: flags cross the bus, rows do not.  The (point, target) -> residual map and the hosts' runs are rebuilt
 * from those copies by the next eds_win_accumulate / eds_wsv_* call, as before.
 *
 * Conventions are those of eds_hip_winsolve.h: plain pointers, EDS_OK or a negative eds_status, eds_last_error() for the text.  Every
 * call returns when its results are on the device (tables) or the host (counts).
 *  - EDS_ERR_INVALID: a NULL handle or required argument, on_device that is neither 0 nor 1, a device pointer that eds_dev_check_range
 *    (include/eds_hip_device.h) refuses over the n or m int32 words that will be read.
 *    eds_wed_marginalize_frame: F outside 3 .. 8, a frame outside 0 .. F - 1, an HM, bM or prior that is not finite.
 *    eds_wed_insert_activated: an eds_imm of another device or another H x W, or whose selection does not cover exactly the frames
 *    the window holds.
 *  - EDS_ERR_STATE: eds_wed_get asked for the idepth backup when no eds_wsv state was ever set; eds_wed_marginalize_frame without a
 *    valid eds_wsv state (the reference asserts EFDeltaValid and EFAdjointsValid; F is that state's), or with a point still hosted by
 *    the frame (the reference asserts); eds_wed_insert_activated without a fit, or with a result beyond max_points / max_residuals.
 *  - EDS_ERR_NOT_USABLE: eds_wed_marginalize_frame met a pivot that is exactly 0, or a result that is not finite.
 *  Nothing is queued and nothing changes on any of these, the tables included.
 * The table edits are integers and copies only; the one place that rounds, marginalizeFrame's arithmetic, has one fixed order stated
 * below and uses no floating-point atomic.  So a run repeats exactly, and the host restatement edswed:: (csrc/eds_winedit.hpp) gives
 * the same bits.
 *
 * MARGINALIZEFRAME'S ARITHMETIC, fp64, one workgroup, the matrix in LDS.  N = 4 + 8 F, nd = N - 8, io = 4 + 8 frame.
 *  1. The frame's block moves to the end (:516-536), exact data movement: P(i) = i below io, i + 8 from io to nd - 1, io + (i - nd)
 *     from nd on; H_ij = HM[P(i)][P(j)], b_i = bM[P(i)].  The last frame takes no branch in the reference: P is the identity.
 *  2. H_(nd+k)(nd+k) += prior[k] and b_(nd+k) += prior[k] * delta_prior[k], k = 0 .. 7: one product and one add (:540-541).
 *  3. S_i = sqrt(|H_ii| + 10), SI_i = 1 / S_i (:548-549).
 *  4. H_ij <- (SI_i * H_ij) * SI_j, b_i <- SI_i * b_i (:556-557).
 *  5. hpi = the inverse of the trailing 8 x 8 block (:560-563).  The reference's two lines hpi = 0.5f * (hpi + hpi) are exact no-ops
 *     (x + x and its half are exact).  The inverse is a STATED one, as the solve's LDLT is stated (Eigen's vectorised LU cannot be
 *     pinned): an LU with partial pivoting by one thread.  For k = 0 .. 7 the pivot is the row r >= k of largest |a_rk|, the LOWEST r on
 *     a tie; rows k and r change places whole; l_rk = a_rk / a_kk (L is unit-lower) and a_rc <- a_rc - l_rk * a_kc for r, c > k.  Then,
 *     for each of the eight columns e of I (its rows permuted as the pivoting permuted them): y_i = rhs_i - (sum over j < i of
 *     l_ij y_j), i ascending, and x_i = (y_i - (sum over j > i of u_ij x_j)) / u_ii, i descending; every sum starts at 0.0 and runs in
 *     ascending j, then ONE subtraction.  hpi_ie = x_i.  A pivot that is exactly 0, or an entry that is not finite: EDS_ERR_NOT_USABLE.
 *  6. bli_ik = sum over j = 0 .. 7 of B_ji hpi_jk from 0.0 in ascending j; B is the bottom-left 8 x nd block (:566).
 *  7. T_ij = A_ij - (sum over k = 0 .. 7 of bli_ik B_kj): the sum first, from 0.0 in ascending k, then one subtraction; the same for b
 *     with the tail of b (:567-568).
 *  8. H_ij <- (S_i * T_ij) * S_j, b_i <- S_i * b_i (:571-572).
 *  9. HM'_ij = 0.5 * (H_ij + H_ji), so HM' is exactly symmetric; bM'_i = b_i (:575-576).  An entry that is not finite:
 *     EDS_ERR_NOT_USABLE.
 * The host restatement edswed::marg_frame_body (csrc/eds_winedit.hpp) is the same code, run by one thread.
 *
 * An eds_wsv state stays valid over both removals and over an insert: have_step / have_backup keep their meaning for the survivors, the frame-sized
 * results of the last solve (x, HFinal, bFinal, xAd) are untouched.  The window's linearized mark is kept too: eds_win_apply after
 * an edit applies the surviving residuals' new states.
 */
#ifndef EDS_HIP_WINEDIT_H_
#define EDS_HIP_WINEDIT_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip_immature.h"
#include "eds_hip_winsolve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_WINEDIT_ABI_VERSION 1
int eds_wed_abi_version(void);

/* what eds_wed_get reads back — the rows no getter of the other two headers returns; meant for tests and debugging: a running back
 * end never needs it — any pointer may be NULL; m residuals, n points */
typedef struct eds_wed_out {
    int32_t* point;                               /* m */
    int32_t* target;                              /* m */
    int32_t* res_first;                           /* n + 1: point p's residuals are res_first[p] .. res_first[p + 1] - 1 */
    int32_t* host;                                /* n */
    float* uv;                                    /* n x 2 */
    float* color;                                 /* n x 8 */
    float* weights;                               /* n x 8 */
    float* idepth_zero_scaled;                    /* n */
    float* deltaF;                                /* n */
    float* idepth_backup;                         /* n; needs an eds_wsv state to have been set once; 0 while no backup holds */
} eds_wed_out;

/* dropResidual for the residuals with select[r] != 0 (m int32 entries, host memory, or device memory with on_device = 1).
 * select == NULL: every residual whose state is not IN (0) goes — what DSO's optimiser loop and removeOutliers drop.  Points are never
 * removed here: a point may end with an empty run.  removed_out (may be NULL): the residuals removed. */
int eds_wed_remove_residuals(eds_win* win, const int32_t* select, int on_device, int32_t* removed_out);
/* dropPointsF and the removePoint half of marginalizePointsF: the points with flag[p] != 0 (n int32 entries, host or device memory)
 * go with all their residuals.  Meant to follow eds_wsv_marginalize_points with the same array.  A host whose run becomes empty is
 * legal.  removed_points_out, removed_residuals_out: may be NULL. */
int eds_wed_remove_points(eds_win* win, const int32_t* flag, int on_device, int32_t* removed_points_out, int32_t* removed_residuals_out);
/* EnergyFunctional::marginalizeFrame (:498-610) and the frame's removal from the window.  The arithmetic is the nine steps above: HM
 * (N x N), bM (N), prior and delta_prior (8 each, the frame's) are host pointers, row-major, finite; HM_out is nd x nd, bM_out nd; they
 * may alias the inputs (everything is read before anything is written).  The tables: every residual whose target is `frame` is
 * removed (FullSystem drops them before the call), hosts and targets above `frame` go down by one, the image planes of the frames above
 * `frame` move down one slot by device copies on the window's stream and the set-marks of the frames follow (slot F - 1 ends unset:
 * the next keyframe's image goes there).  The eds_wsv state becomes invalid, because F changed: set it again with eds_wed_set_state,
 * which keeps the per-point and per-residual rows. */
int eds_wed_marginalize_frame(eds_win* win, int frame, const double* prior, const double* delta_prior, const double* HM, const double* bM,
                              double* HM_out, double* bM_out);
/* eds_wsv_set_state with the per-point arrays taken from the device instead of the host, by the same code: deltaF[p] = inv *
 * idepth_scaled[p] - inv * idepth_zero_scaled[p] with inv = 1.0f / scale_idepth (setDeltaF, :190).  Where a state was set since the
 * last eds_win_set_points / eds_win_set_residuals — valid still, or invalidated by eds_wed_marginalize_frame — priorF, is_linearized
 * and res_toZeroF are KEPT as they are (DSO keeps a residual's linearization across keyframes); otherwise they are 0, as
 * eds_wsv_set_state leaves them.  The L sums, the steps and resApprox are cleared either way: the next solve forms them again. */
int eds_wed_set_state(eds_win* win, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior,
                      const double* delta_prior, const double* cPrior, const double* cDelta);
/* The ACTIVATED points of the eds_imm's last eds_act_optimize (include/eds_hip_activate.h) enter the window, straight from the device
 * arrays eds_act_get_activated reads; no row is read back (the candidates' flags are).  Same device and H x W and a selection whose
 * n_hosts equals the number of frames the window holds (slots 0 .. F - 1 set), else EDS_ERR_INVALID; no fit, or a result beyond
 * max_points / max_residuals, EDS_ERR_STATE; nothing changes on either.  For each host the host's own points come first, in order, then
 * its activated points in index order: a stable merge that keeps the grouping.  A new point has the immature point's uv, color and
 * weights, idepth_scaled = idepth_zero_scaled = the fitted idepth times the eds_act scale_idepth (what eds_act_get_activated returns),
 * and priorF, deltaF, the L sums, step and backup 0.  It has one residual per target t whose fitted residual state is IN, in
 * ascending t, exactly as eds_win_set_residuals leaves a residual with state IN and energy 0: new state OUTLIER, not active, J zero,
 * not linearized.  The window's linearized mark is cleared: eds_win_apply is EDS_ERR_STATE until the next eds_win_linearize.  An
 * eds_wsv state stays valid.  inserted_points_out, inserted_residuals_out: may be NULL. */
int eds_wed_insert_activated(eds_win* win, eds_imm* imm, int32_t* inserted_points_out, int32_t* inserted_residuals_out);
/* the point and residual counts and the points per host frame; any pointer may be NULL */
int eds_wed_counts(eds_win* win, int32_t* n, int32_t* m, int32_t* per_host /* [8] */);
int eds_wed_get(eds_win* win, const eds_wed_out* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_WINEDIT_H_ */
