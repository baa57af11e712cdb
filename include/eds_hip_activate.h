/* eds_hip_activate.h — activation of DSO's immature points, on the device, over the eds_imm of eds_hip_immature.h: the coarse distance
 * map of where active points project into the newest keyframe (CoarseDistanceMap::makeDistanceMap, growDistBFS, addIntoDistFinal,
 * reference src/tracking/CoarseTracker.cpp:731-882), the candidate rule over every immature point in order, and the Gauss-Newton fit of
 * each chosen point's inverse depth against every other frame of the window (ImmaturePoint::linearizeResidual,
 * src/tracking/ImmaturePoint.cpp:529-596, with projectPoint and derive_idepth of src/tracking/ResidualProjections.h:35-86).  The symbols
 * are exported by libeds_hip.so.  The state hangs off the eds_imm: the first call that needs it allocates it, eds_imm_destroy releases
 * it.  A process that never calls eds_act_* allocates and launches nothing of this, and every other call returns the bits it returned.
 *
 * WHAT IS PINNED TO WHAT.  The reference tree holds the callees, not the two loops that drive them (activatePointsMT and
 * optimizeImmaturePoint live in DSO's FullSystem, which EDS replaces).  Both loops are therefore STATED here; parity with EDS's own
 * caller is unpinned for the loops and pinned to the reference text for everything they call.
 *
 * Conventions are those of eds_hip_immature.h: plain pointers, EDS_OK or a negative eds_status, eds_last_error() for the text,
 * eds_dev_check_range on everything handed over as device memory, every call returns when its results are on the host, nothing
 * changes on an error, no floating-point atomic anywhere, a run repeats exactly.
 *  - EDS_ERR_INVALID: NULL handle or required argument, newest / n_hosts / host out of range, n_hosts above EDS_ACT_MAX_FRAMES, a
 *    KRKi1 / Kt1 / precalc / threshold that is not finite, active points whose hosts are out of range or not grouped by host, a
 *    parameter eds_act_set_params refuses, a calibration that is not finite and positive in fx, fy or a level-1 map below 3 x 3, a
 *    device range eds_dev_check_range refuses.
 *  - EDS_ERR_STATE: no calibration yet; eds_act_select before a map exists; eds_act_optimize before a selection (or twice on one);
 *    eds_act_get_distance_map before a map; a frame of 0 .. n_hosts - 1 without an image.  eds_imm_set_host_images and
 *    eds_imm_create_points drop map, selection and fit.
 *
 * The frames of the window are the host frames 0 .. F - 1 of the eds_imm, in window order; their stored level-0 planes
 * {colour, dx, dy} are the dI that linearizeResidual samples.  No target image is involved.
 *
 * 1. THE DISTANCE MAP (level 1: w1 = W >> 1, h1 = H >> 1).  Every cell 1000.  For each active point not hosted by `newest`,
 *    ptp = (KRKi1[h] row . (u, v, 1), summed left to right) + Kt1[h] * idepth_scaled; u1 = (int)(ptp0 / ptp2 + 0.5f), v1 likewise; kept
 *    when u1 > 0 && v1 > 0 && u1 < w1 && v1 < h1: its cell becomes 0 and a seed.  Defined where the reference is undefined: a quotient
 *    that is not finite or beyond +-2^20 is outside (the float-to-int conversion is never reached).  growDistBFS, which is
 *    level-synchronous by construction: rounds k = 1 .. 39; round k takes the cells newly set in round k - 1 (the seeds for k = 1) and,
 *    from each that is not on the map's outer ring, sets every neighbour whose value is > k to k — the 8-neighbourhood for odd k, the
 *    4-neighbourhood for even k.  Ring cells are reached, never expanded.  Values are integers 0 .. 39 or 1000 and do not depend on
 *    list order or duplicate seeds.
 *
 * 2. THE CANDIDATE RULE walks hosts 0 .. n_hosts - 1 except `newest`, and within a host its live points in index order; the order
 *    matters, every chosen point changes the map the next one reads.
 *      a  !isfinite(idepth_max) or lastTraceStatus OUTLIER                                   -> DELETED_UNTRACED
 *      b  canActivate false: DELETED_CANNOT if the host is flagged or the status is OOB, else   KEPT_CANNOT
 *         canActivate = status in {GOOD, SKIPPED, BADCONDITION, OOB} && lastTracePixelInterval < max_trace_pixel_interval &&
 *                       quality > min_trace_quality && (idepth_max + idepth_min) > 0
 *      c  ptp = KRKi1 . (u, v, 1) + Kt1 * (0.5f * (idepth_max + idepth_min)); the cell as above; outside the map -> DELETED_OUT_OF_MAP
 *      d  dist = map[u1 + w1 v1] + (ptp0 - floorf(ptp0))   (the undivided ptp0 is DSO's);
 *         dist >= current_min_act_dist * my_type: addIntoDistFinal(u1, v1)                   -> CHOSEN
 *      e  otherwise                                                                          -> KEPT_TOO_CLOSE
 *    addIntoDistFinal sets the cell to 0 and runs growDistBFS from that one seed by the same round rule (a cell is taken only if its
 *    value is > k; only cells taken in a round expand in the next): NOT min(old, distance from the new seed) — a path can be cut by a
 *    cell that was already close.  One workgroup walks this loop on the device; the host form is the same text with one thread.
 *
 * 3. THE FIT of every CHOSEN point.  Its residuals are the frames 0 .. n_hosts - 1 except its host, in that order, each starting with
 *    state IN, energy 0.  idepth = (idepth_max + idepth_min) * 0.5f.
 *    eval(idepth, slack): Hdd = bd = 0.0f, E = 0.0f; for each residual in order E = (float)((double)E + (double)linearizeResidual(...)).
 *    linearizeResidual is the reference's: a residual whose state is OOB sets new_state OOB, returns its stored energy, adds nothing;
 *    otherwise taps 0 .. 7 in order, a tap whose projectPoint fails (!(drescale > 0) first, then the 1.1f / wM3G box) or whose sample
 *    is not finite sets new_state OOB and returns the STORED energy — what earlier taps of that residual already added to Hdd and bd
 *    STAYS added.  Per tap hw = fabsf(r) < huber ? 1 : huber / fabsf(r); energy += ((((w w) hw) r) r) (2 - hw); d = derive_idepth;
 *    hw *= w w; Hdd += (hw d) d; bd += (hw r) d.  After the last tap energy > energyTH * slack clamps the energy and gives OUTLIER, else
 *    IN; new_energy is the energy.  huber is the eds_imm's own huber_th.  The sample is getInterpolatedElement33 with the validity rule
 *    and the weight order of eds_hip_immature.h; fxli = 1.0f / fx, wM3G = W - 3.
 *    The loop:  eval(idepth, 1000), every residual takes its new state and energy.  !isfinite(E) or Hdd < min_idepth_h_act: KEPT_WEAK.
 *    lambda = 0.1f; for it < gn_its: H = Hdd * (1 + lambda); step = (float)((1.0 / (double)H) * (double)bd); new = idepth - step;
 *    eval(new, 1) gives E', Hdd', bd'; !isfinite(E) — the OLD E, as DSO writes it — or Hdd' < min_idepth_h_act: KEPT_WEAK; E' < E: take
 *    idepth, Hdd, bd, E and every residual's new state and energy, lambda *= 0.5f; otherwise lambda *= 5 and the residuals' new_* are
 *    left; break when (double)fabsf(step) < 0.0001 * (double)idepth with the idepth that now holds.  Then !isfinite(idepth) or fewer
 *    than min_obs residuals IN: DROPPED; otherwise ACTIVATED with idepth as both idepth and idepth_zero.  A live point's energyTH is
 *    finite (eds_hip_immature.h), so the last check of PointHessian's constructor cannot fire.
 *    AFTERWARDS these points leave the immature set — ACTIVATED, DROPPED, KEPT_WEAK while their status is OOB, every DELETED_* — and
 *    are dead exactly as alive = 0 points are.  Everything else is untouched bit for bit.
 *    Eight lanes evaluate the taps of one residual, eight residuals share a wavefront, more targets loop; the running sums are then
 *    folded in the serial order above.
 */
#ifndef EDS_HIP_ACTIVATE_H_
#define EDS_HIP_ACTIVATE_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip_immature.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_ACTIVATE_ABI_VERSION 1
int eds_act_abi_version(void);

#define EDS_ACT_MAX_FRAMES 64

typedef enum eds_act_fate {
    EDS_ACT_NONE = 0,               /* a dead point, or a point of `newest` */
    EDS_ACT_DELETED_UNTRACED = 1,
    EDS_ACT_DELETED_CANNOT = 2,
    EDS_ACT_KEPT_CANNOT = 3,
    EDS_ACT_DELETED_OUT_OF_MAP = 4,
    EDS_ACT_CHOSEN = 5,             /* between eds_act_select and eds_act_optimize */
    EDS_ACT_KEPT_TOO_CLOSE = 6,
    EDS_ACT_KEPT_WEAK = 7,
    EDS_ACT_DROPPED = 8,
    EDS_ACT_ACTIVATED = 9
} eds_act_fate;
#define EDS_ACT_NUM_FATES 10

typedef struct eds_act_params {
    float min_idepth_h_act;                  /* setting_minIdepthH_act 100 */
    int32_t gn_its_on_point_activation;      /* 3; 0 .. 16 */
    float min_trace_quality;                 /* 3 */
    float max_trace_pixel_interval;          /* 8 */
    int32_t min_obs;                         /* 1; 0 .. EDS_ACT_MAX_FRAMES */
    float scale_idepth;                      /* SCALE_IDEPTH 1; > 0 */
} eds_act_params;
void eds_act_params_default(eds_act_params* p);
/* every float finite, scale_idepth > 0, the integers in range */
int eds_act_set_params(eds_imm* imm, const eds_act_params* p);
int eds_act_get_params(eds_imm* imm, eds_act_params* p);

/* fx, fy finite and > 0, cx, cy finite; W >> 1 and H >> 1 at least 3 */
int eds_act_set_calib(eds_imm* imm, float fx, float fy, float cx, float cy);

/* KRKi1[h] = K[1] * R * Ki[0] (row-major 3 x 3) and Kt1[h] = K[1] * t of host h into frame `newest`, n_hosts of each.  The active points:
 * n_active rows {u, v, idepth_scaled} with active_host[i], grouped by host; on_device = 0: both in host memory, 1: both in device
 * memory, range-checked. */
int eds_act_make_distance_map(eds_imm* imm, int newest, int n_hosts, const float* KRKi1, const float* Kt1, int n_active,
                              const int32_t* active_host, const float* active_uv_idepth, int on_device);
/* h1 x w1 floats */
int eds_act_get_distance_map(eds_imm* imm, float* out);

/* flagged_for_marginalization: n_hosts bytes (NULL: none).  counts_out (EDS_ACT_NUM_FATES ints, may be NULL): live points per fate. */
int eds_act_select(eds_imm* imm, int newest, int n_hosts, const float* KRKi1, const float* Kt1, const uint8_t* flagged_for_marginalization,
                   float current_min_act_dist, int32_t* counts_out);

/* precalc[(host * n_hosts + target) * 14]: PRE_RTll (row-major 9), PRE_tTll (3), PRE_aff_mode (2) — the NON-_0 values of
 * FrameFramePrecalc::set; the diagonal is not read.  n_hosts is the selection's.  counts_out as above, after the fit. */
int eds_act_optimize(eds_imm* imm, int n_hosts, const float* precalc, int32_t* counts_out);

/* per point of `host` (n of eds_imm_num_points; any output may be NULL); res_state / res_energy are n x n_hosts of the selection, the
 * column of the point's own host and every column of a point that was not fitted -1 / 0; idepth, energy, hdd, bd are 0 for those */
int eds_act_get(eds_imm* imm, int host, int32_t* fate, float* idepth, float* energy, float* hdd, float* bd, int32_t* res_state, float* res_energy);

/* the ACTIVATED points in (host, index) order, at most cap of them (*n: how many there are): uv n x 2, type, idepth (times scale_idepth:
 * idepth_scaled and idepth_zero_scaled alike), color n x 8, weights n x 8, target_mask bit t: the residual towards frame t is IN.
 * Any output array may be NULL. */
int eds_act_get_activated(eds_imm* imm, int cap, int* n, int32_t* host, int32_t* index, float* uv, float* type, float* idepth, float* color,
                          float* weights, uint64_t* target_mask);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_ACTIVATE_H_ */
