/* eds_hip_klt.h — the KLT point trackers of EDS on the device: Tracker::trackPoints and Tracker::trackPointsPyr (reference
 * src/tracking/Tracker.cpp:378-488) for the points a tracker handle (include/eds_hip.h) already holds.
 *
 * One call re-projects the points at each slot's solved pose and erases the ones that left the frame (getCoord(true), as
 * eds_trk_update_points(delete_out_points = 1)), splats the keyframe gradients at the warped coordinates (drawValuesPoints,
 * bilinear, blurred 3 x 3 with sigma 0.5), cuts the reflect-101 windows of both gradient images and of the event frame the
 * solve read (splitImageInPatches), and solves kltTracker's 2 x 2 system per point, per pyramid level for the pyr variant.
 * The results stay in HBM: per slot, fp64 planes tracks (kf->tracks) and flow (kf->flow), which eds_depth_update reads with
 * EDS_DEPTH_DEVICE_TRACKS (include/eds_hip_depth.h).  The symbols are exported by libeds_hip.so.
 *
 * Conventions are those of eds_hip.h: plain pointers and sizes, caller-owned fp64 host buffers, EDS_OK or a negative eds_status.
 * Every call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a radius outside 0 .. 31, a level count outside 1 .. 5, bad slot ranges or strides, null outputs where one
 *    is needed.
 *  - EDS_ERR_STATE: a slot without keyframe or event frame, a slot without device tracks (eds_klt_get), or a batch in flight
 *    (eds_trk_optimize_batch without eds_trk_sync).  Nothing changes on an error.
 *
 * State:
 *  - the tracks and flow planes are allocated (zero) by the first eds_klt_track_points* of a handle.  From then on every
 *    eds_trk_update_points(_batch) writes getCoord's re-projection tracks into them and, erasing points, compacts the flow the
 *    same way (KeyFrame::erasePoint, KeyFrame.cpp:1060-1106).  eds_trk_set_keyframe / eds_trk_build_keyframe* zero them
 *    (KeyFrame::create, KeyFrame.cpp:447-448).  A handle that never calls KLT allocates and launches nothing of this.
 *  - trackPoints assigns the flow and adds it to the track; trackPointsPyr adds it to both.
 *
 * Numerics: fp64 throughout, no FMA contraction; every splat pixel sums its contributions in ascending point index, as the
 * reference's loop does.  kltTracker's five sums are tree reductions, not cv::sum's running sum (same terms, other rounding).
 * Zero gradients over a window give inf / NaN, propagated like the reference's.  A point exactly on the right or bottom edge
 * (x == cols, y == rows) is kept by getCoord; the reference's cv::Rect then throws, here the window keeps reflecting
 * (cv::borderInterpolate, reflect-101, repeated while the window is wider than the image).  A point whose coordinates are not
 * finite splats nothing and gets a NaN flow.
 */
#ifndef EDS_HIP_KLT_H_
#define EDS_HIP_KLT_H_

#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_KLT_ABI_VERSION 1
int eds_klt_abi_version(void);

/* Tracker::trackPoints(event_frame, patch_radius) for slots first .. first + count - 1, each against the event frame its solve
 * read (its own or the one it shares: eds_trk_share_event_frame).  patch_radius 0 .. 31 (the reference's default is 7).
 * Outputs as eds_trk_update_points_batch: alignment b writes points from index b * stride (pixels, N x 2 for the xy arrays),
 * n_kept[b] is its point count after the erasure; any output may be NULL (stride is then not checked).
 *   coord_xy   getCoord's warped coordinates
 *   tracks_xy  kf->tracks after the call: coord - keyframe pixel + flow
 *   flow_xy    kf->flow after the call
 *   kept_index the original index of each kept point */
int eds_klt_track_points(eds_trk* h, int first, int count, int patch_radius, int stride, double* coord_xy, double* tracks_xy,
                         double* flow_xy, int32_t* kept_index, int* n_kept);
/* Tracker::trackPointsPyr(event_frame, num_level): num_level 1 .. 5, radius (3 * 2^(L-1) + L) / 2 = 2, 4, 7, 14, 26; the flow
 * of level j enters with weight 1 / 2^j / 2^j and is added to both kf->flow and kf->tracks.  Outputs as above. */
int eds_klt_track_points_pyr(eds_trk* h, int first, int count, int num_level, int stride, double* coord_xy, double* tracks_xy,
                             double* flow_xy, int32_t* kept_index, int* n_kept);
/* the device's kf->tracks and kf->flow of one slot, N x 2 each (either may be NULL, not both) */
int eds_klt_get(eds_trk* h, int slot, double* tracks_xy, double* flow_xy);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_KLT_H_ */
