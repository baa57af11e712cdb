/* eds_hip_epiline.h — Tracker::trackPointsAlongEpiline of EDS on the device (reference src/tracking/Tracker.cpp:490-553) for the
 * points a tracker handle (include/eds_hip.h) already holds, feeding DepthPoints::update(T_kf_ef, kf_coord, ef_coord)
 * (src/mapping/DepthPoints.cpp:93-135) without a host round trip.
 *
 * One call, per slot:
 *  1. the model image kf->getModel(linearVelocity(), angularVelocity(), "bilinear") (KeyFrame.cpp:1358-1423): per point
 *     f = compute_flow(norm_coord, v, w, mu) (Utils.hpp:165-173), m = -(g . f) / sqrt(1e-3 + sum m^2), splatted bilinearly at the
 *     keyframe pixels in point order (drawValuesPoints, Utils.cpp:124-193), blurred 3 x 3 with sigma 0.5 (reflect-101).  A keyframe
 *     pixel outside the frame is splatted as there: a corner outside carries weight 0, so a pixel with x in (-1, 0) adds its x1
 *     corners to column 0 (y likewise to row 0), and one with x <= -1, x >= cols, y <= -1 or y >= rows adds nothing;
 *  2. the templates: splitImageInPatches(model, kf->coord, r, border_type, border_value) (Utils.cpp:608-633), each (2r+1)^2 patch
 *     in fp32, placed at the TRUNCATED keyframe pixel;
 *  3. the search image: copyMakeBorder(event_frame, r, border_type, border_value) in fp32;
 *  4. per point, both eds::utils::matchTemplate calls (Utils.cpp:992-1023): p_ssd = the minimum of TM_SQDIFF_NORMED, p_ncc = the
 *     maximum of TM_CCORR_NORMED, each over the H x W result (an event-frame pixel);
 *  5. the cull: a point with |‖p_ssd‖ - ‖p_ncc‖| > 5 is erased (kf->erasePoint, KeyFrame.cpp:1060-1106); the kept points' p_ssd
 *     are the result, and stay on the device as the slot's ef plane.
 *
 * Scores (our reading of OpenCV's normed-score rule; E = sum P^2 over the window, S = sum T^2, C = sum P T, t = sqrt(E) sqrt(S)):
 *   CCORR_NORMED   C / t if |C| < t, +-1 if |C| < 1.125 t, else 0;
 *   SQDIFF_NORMED  num = max(E - 2C + S, 0): num / t if num < t, else 1.
 * Scores are compared as fp32 (OpenCV's CV_32F result), -0 == +0, and the first position in row-major order wins a tie
 * (cv::minMaxLoc).  C is accumulated in fp32 on the device, E and S are exact fp64 sums of fp32 squares rounded to fp32.
 *
 * Deliberate deviations from the reference:
 *  - the match rectangles are not drawn.  The reference's cv::Mat img_display = img is a shallow copy, so every match zeroes a
 *    2-px outline in the search image that p_ncc of the same point and every later point then see.  Here every point is matched
 *    against the clean padded frame: the result does not depend on point order.
 *  - the stdout prints, the /tmp PNG writes, computeCorrespondEpilines and getFMatrix (computed, never read) are dropped.
 *  - cv::normalize(NORM_MINMAX) before cv::minMaxLoc is not reproduced: it is monotone; only its fp32 rounding could merge values
 *    within an ulp of the extremum.
 *  - a method without any finite score reports (-1, -1), and the point fails the cull.
 *  - inputs are what the slot holds: its fp32 gradients, the fp64 mu of its seeds when seeded (include/eds_hip_depth.h) and else its
 *    fp32 inverse-depth plane, the keyframe pixel as an integer cell plus an fp32 fraction, and its fp32 event frame (the frame its
 *    solve reads, its own or the one it shares).
 *
 * Conventions are those of eds_hip.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status.  Every
 * call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a radius outside 0 .. 15, an unknown border type, a border value outside 0 .. 255, bad slot ranges or strides.
 *  - EDS_ERR_STATE: a slot without keyframe or event frame, a batch in flight (eds_trk_optimize_batch without eds_trk_sync), and for
 *    eds_epi_get / eds_epi_depth_update a slot whose ef plane is not current.  Nothing changes on an error.
 *
 * State:
 *  - the ef plane (fp64, [2][B][Np]) and the work buffers are allocated by the first eds_epi_* call of a handle.  A handle that never
 *    calls eds_epi_* allocates and launches nothing of this.
 *  - after eds_epi_track_points the ef plane is index-aligned with the slot's points: the kept points' p_ssd with erase = 1, every
 *    point's with erase = 0.  Any later change of the slot's point set or keyframe makes it stale: eds_trk_set_keyframe,
 *    eds_trk_build_keyframe*, eds_trk_update_points* with delete_out_points = 1, eds_klt_track_points*.
 *  - erasing leaves the slot exactly as getCoord's compaction (eds_trk_update_points) leaves it after erasing the same points: the
 *    per-point planes, residuals, per-block statistics, seeds, and the KLT's tracks and flow when they exist.
 */
#ifndef EDS_HIP_EPILINE_H_
#define EDS_HIP_EPILINE_H_

#include <stdint.h>

#include "eds_hip.h"
#include "eds_hip_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_EPILINE_ABI_VERSION 1
int eds_epi_abi_version(void);

/* cv::BORDER_* values, so a caller passes OpenCV's constant through; BORDER_DEFAULT = 4 */
enum eds_epi_border {
    EDS_EPI_BORDER_CONSTANT = 0,
    EDS_EPI_BORDER_REPLICATE = 1,
    EDS_EPI_BORDER_REFLECT = 2,
    EDS_EPI_BORDER_REFLECT_101 = 4
};

/* trackPointsAlongEpiline(event_frame, patch_radius, border_type, border_value) for slots first .. first + count - 1.
 * patch_radius 0 .. 15 (the reference's default is 7); border_value 0 .. 255, used by CONSTANT only, for the model and the search
 * image alike.  erase = 1 is the reference's behaviour; with erase = 0 the slot keeps all its points and the outputs are the same.
 * Per ORIGINAL point i of alignment b, at b * stride + i:
 *   ssd_xy  p_ssd (x, y), int32 pairs        ncc_xy  p_ncc (x, y)        scores  the two winning fp32 scores (ssd, ncc) as fp64
 * Per KEPT point k of alignment b, at b * stride + k (what the reference returns):
 *   ef_xy   p_ssd as fp64 pixels             kept_index  the original index             n_kept[b]  the number of kept points
 * Every output may be NULL (stride is then not checked). */
int eds_epi_track_points(eds_trk* h, int first, int count, int patch_radius, int border_type, int border_value, int erase,
                         int stride, int32_t* ssd_xy, int32_t* ncc_xy, double* scores,
                         double* ef_xy, int32_t* kept_index, int* n_kept);
/* the device ef plane of one slot, N x 2 */
int eds_epi_get(eds_trk* h, int slot, double* ef_xy);
/* getModel(v, w, "bilinear", 0.5) at the slot's current velocity and points: H x W fp64, row-major */
int eds_epi_get_model(eds_trk* h, int slot, double* model);
/* DepthPoints::update(T_kf_ef, kf->coord, ef_coord) with ef_coord = the device ef plane: bit-identical to eds_depth_update(...,
 * EDS_DEPTH_EF_COORD, xy = the same coordinates from the host, kf_xy = NULL, ...).  T_kf_ef, filter and out as there. */
int eds_epi_depth_update(eds_trk* h, int first, int count, const double* T_kf_ef, int filter, eds_depth_summary* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_EPILINE_H_ */
