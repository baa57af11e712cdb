/* eds_hip_kfpoints.h — what EDS's KeyFrame does to its own point set, on the device, for the points a tracker handle (include/eds_hip.h)
 * already holds: KeyFrame::pointsRefinement (reference src/tracking/KeyFrame.cpp:1031-1058), KeyFrame::cleanPoints (:1566-1587),
 * KeyFrame::erasePoint (:1060-1106), KeyFrame::num_points for needNewKF / needNewKFImageCriteria (:1552-1564), and the keyframe switch:
 * getDepthMap() (:1220-1237) moved by a pose and pushed through IDepthMap::fromPoints (src/mapping/Types.hpp:248-275).
 *
 * pointsRefinement.
 *  - Window.  The reference pads the event frame by r and takes cv::Rect(p.x, p.y, 2r+1, 2r+1) of the padded image
 *    (splitImageInPatches, Utils.cpp:608-633): the (2r+1)^2 window is centred on the TRUNCATED keyframe pixel.  The pixel is what the
 *    slot holds, an integer cell plus an fp32 fraction, truncated as the epiline templates truncate it (a pixel that fx ((u - cx) / fx)
 *    + cx put 1e-13 below an integer u holds the fraction 1.0f and comes back as u).  A tap outside the frame follows the border rule
 *    (cv::borderInterpolate, repeated while outside; CONSTANT: border_value), also for a truncated pixel that itself lies outside the
 *    frame, where OpenCV would throw: here it is defined and never reads out of bounds.  (A truncated coordinate beyond +-2^20 is
 *    taken as +-2^20.)
 *  - Decision.  Taps are the slot's stored fp32 values; min and max ignore NaN taps (fminf / fmaxf); a point is erased iff
 *    fabs((double)max - (double)min) < event_diff, in fp64.  A window without a finite tap has a NaN range and is kept.  Every operation
 *    is exact or correctly rounded: the erased set equals that of the same rule applied to the frame eds_trk_get_event_frame returns,
 *    bit for bit.
 *  - The stored frame is event_frame[level] divided by its Frobenius norm unless cfg.nc (include/eds_hip.h): a threshold given in event
 *    units is event_diff / norm here.
 *  - The frame is the one the slot's solve reads: its own or the one it shares (eds_trk_share_event_frame).
 *
 * cleanPoints compares the stored fp32 weight, widened to fp64, < w_norm_thr.
 *
 * After any erasing call a slot is exactly what the epiline cull (include/eds_hip_epiline.h) leaves after erasing the same points: the
 * per-point planes, residuals, per-block statistics and seeds are compacted in order, and the KLT's tracks and flow where they exist;
 * the epiline's ef plane goes stale.  A slot may end with 0 points: it then holds no keyframe until the next eds_trk_set_keyframe /
 * eds_trk_build_keyframe*.
 *
 * num_points (KeyFrame::num_points, per slot): eds_trk_set_keyframe, eds_dev_set_keyframes and eds_pyr_* set it to N;
 * eds_trk_build_keyframe* sets it to the candidate count BEFORE cleanPoints (candidatePoints assigns it, :820; cleanPoints does not
 * touch it); eds_kfp_refine_points with erase = 1 sets it to the kept count (:1056).  Nothing else changes it.
 *
 * Projection, all in fp64 without FMA contraction, in this order:
 *   u, v = cell + (double)fraction;  mu = the seed's fp64 mu when the slot is seeded (include/eds_hip_depth.h), else (double) of the fp32
 *   inverse-depth plane;  d = 1 / mu;  X = d ((u - cx) / fx);  Y = d ((v - cy) / fy);  Z = d;
 *   X' = R00 X + R01 Y + R02 Z + t0 summed left to right, Y' and Z' likewise, R formed from q on the host in fp64;
 *   px = fxd (X' / Z') + cxd;  py = fyd (Y' / Z') + cyd;  idp' = 1 / Z';
 *   kept iff px >= 0 && px < dst_W && py >= 0 && py < dst_H, order preserved.
 * A point with Z' <= 0 that still lands in the frame is kept with its non-positive idp': the reference does not test for it either.
 *
 * Conventions are those of eds_hip_epiline.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status.
 * Every call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, bad slot ranges or strides (a stride is checked only when an output that uses
 *    it is given), a radius outside 0 .. 15, an unknown border type, a border value outside 0 .. 255, erase other than 0 / 1, a
 *    threshold that is not finite, a pose or intrinsics that are not finite, a zero quaternion or focal length.
 *  - EDS_ERR_STATE: a slot without a keyframe, for eds_kfp_refine_points a slot without an event frame, a batch in flight
 *    (eds_trk_optimize_batch without eds_trk_sync).  Nothing changes on an error.  eds_kfp_counts reads two host fields: it needs
 *    neither a keyframe nor an idle handle.
 * A handle that never calls eds_kfp_* allocates and launches nothing of this.  Results have a fixed order: a batch equals its singles bit
 * for bit and runs repeat exactly.
 */
#ifndef EDS_HIP_KFPOINTS_H_
#define EDS_HIP_KFPOINTS_H_

#include <stdint.h>

#include "eds_hip.h"
#include "eds_hip_epiline.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_KFPOINTS_ABI_VERSION 1
int eds_kfp_abi_version(void);

/* KeyFrame::pointsRefinement(event_frame, event_diff, patch_radius, border_type, border_value) for slots first .. first+count-1,
 * on the frame each slot's solve reads (its own or the one it shares).  patch_radius 0 .. 15 (reference default 11),
 * border_type / border_value as in eds_hip_epiline.h (cv::BORDER_*; value 0 .. 255, CONSTANT only), event_diff finite.
 * erase = 1 is the reference; erase = 0 computes and reports only.
 *   range       per ORIGINAL point i of alignment b, at b*stride+i: max - min of its window, fp64 (NaN: no finite tap)
 *   kept_index  per KEPT point k, at b*stride+k: its original index          n_kept[b]: points left
 * Any output may be NULL. */
int eds_kfp_refine_points(eds_trk* h, int first, int count, double event_diff, int patch_radius, int border_type, int border_value,
                          int erase, int stride, double* range, int32_t* kept_index, int* n_kept);
/* KeyFrame::cleanPoints(w_norm_thr) on the slots' weight planes */
int eds_kfp_clean_points(eds_trk* h, int first, int count, double w_norm_thr, int stride, int32_t* kept_index, int* n_kept);
/* KeyFrame::erasePoint for every i with erase[b*stride+i] != 0 (host bytes; entries beyond a slot's N are ignored) */
int eds_kfp_erase_points(eds_trk* h, int first, int count, int stride, const uint8_t* erase, int32_t* kept_index, int* n_kept);
/* KeyFrame::num_points and coord.size() per slot (needNewKF / needNewKFImageCriteria are one line each on these); a slot without a
 * keyframe reports current = 0.  Either output may be NULL. */
int eds_kfp_counts(eds_trk* h, int first, int count, int* num_points, int* current);
/* getDepthMap() -> T_dst_src * p -> IDepthMap::fromPoints(points, {dst_W, dst_H}, K_dst): the depth map the NEXT keyframe's
 * eds_trk_build_keyframe* takes.  T7: count x {p[3], q_xyzw[4]} of T_dst_src, NULL = each slot's current state (the solved
 * T_ef_kf); K_dst: count x {fx, fy, cx, cy}, NULL = the slot's own; dst_H / dst_W <= 0: the handle's.  Per alignment b, at
 * b*stride: depth_xy (n x 2), depth_idp (n), src_index (n, original index), n_out[b].  The slot is not modified. */
int eds_kfp_project_depth_map(eds_trk* h, int first, int count, const double* T7, const double* K_dst, int dst_H, int dst_W,
                              int stride, double* depth_xy, double* depth_idp, int32_t* src_index, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_KFPOINTS_H_ */
