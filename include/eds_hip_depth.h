/* eds_hip_depth.h — the inverse-depth filter of EDS on the device: eds::mapping::DepthPoints (reference
 * src/mapping/DepthPoints.{hpp,cpp}) for the points a tracker handle (include/eds_hip.h) already holds.
 *
 * The reference keeps one seed [mu, sigma2, a, b] per keyframe point (fp64, DepthPoints.hpp:38,53), updates it after every
 * tracking step from the point's track (DepthPoints.cpp:137-178: triangulation, depth uncertainty, Vogiatzis Gaussian x Beta
 * update) and Tracker::optimize re-reads mu on every call (Tracker.cpp:167).  Here the seeds live in HBM next to the slot's
 * point planes, one fused kernel updates them, and the slot's inverse-depth plane and Gram matrices are refreshed on the device:
 * the next solve reads the filtered depths with no host round trip.  The symbols are exported by libeds_hip.so.
 *
 * Conventions are those of eds_hip.h: plain pointers and sizes, caller-owned fp64 host buffers that only need to live for the
 * call, EDS_OK or a negative eds_status.  Every call here returns when its results are on the host (it waits for the stream).
 *  - EDS_ERR_INVALID: sizes, strides, slot ranges, enums.
 *  - EDS_ERR_STATE: a slot without keyframe, a slot that is not seeded (every call but eds_depth_init), or a batch in flight
 *    (eds_trk_optimize_batch without eds_trk_sync: its poses have not reached the slots yet).  Nothing changes on an error.
 *
 * Interactions with eds_hip.h:
 *  - eds_trk_set_keyframe / eds_trk_build_keyframe* unseed the slot (KeyFrame::setDepthMap seeds a new DepthPoints,
 *    KeyFrame.cpp:1197).
 *  - eds_trk_update_points(_batch) with delete_out_points erases the seeds of the points it erases, in the same order
 *    (KeyFrame::erasePoint, KeyFrame.cpp:1060-1106): seeds stay index-aligned with the planes.  Unseeded slots: unchanged.
 *  - every call here that changes mu leaves the slot exactly as eds_trk_set_idepth(h, slot, N, mu) would: plane = (float)mu,
 *    Gram matrices refreshed in HBM.  eds_trk_set_idepth leaves the seeds alone: until the next call here the plane the
 *    tracker reads may differ from mu.
 */
#ifndef EDS_HIP_DEPTH_H_
#define EDS_HIP_DEPTH_H_

#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_DEPTH_ABI_VERSION 2
int eds_depth_abi_version(void);

/* DepthPoints::init's scalar arguments (DepthPoints.hpp:60-75): the depth range gives mu_range = max - min; threshold is
 * convergence_sigma2_thresh (KeyFrame::setDepthMap passes it, KeyFrame.cpp:1197).  px_noise is the reference's constant 3. */
typedef struct eds_depth_params {
    double min_depth, max_depth;
    double threshold;               /* 100 */
    double init_a, init_b;          /* 2, 5 */
} eds_depth_params;
void eds_depth_params_default(eds_depth_params* prm);

/* init sources */
enum eds_depth_init_source {
    EDS_DEPTH_INIT_CONSTANT = 0,    /* init(K, num_points, ...) (DepthPoints.cpp:59-78): mu = 1/((max-min)/2), sigma2 = mu_range^2 */
    EDS_DEPTH_INIT_HOST = 1,        /* init(K, inv_depth, ...) (:80-99): mu = idp[b * stride + i], sigma2 = mu_range^2 / 36 */
    EDS_DEPTH_INIT_PLANE = 2        /* as HOST from the slot's own fp32 inverse-depth plane (what eds_trk_build_keyframe left):
                                     * NARROWED values, mu = (double)(float)idp */
};
/* Seeds slots first .. first + count - 1 with the slot's current point count and intrinsics (K from the keyframe).  a = init_a,
 * b = init_b.  The seed planes are allocated at the first call of a handle. */
int eds_depth_init(eds_trk* h, int first, int count, const eds_depth_params* prm, int source, const double* idp, int stride);

/* where the event-frame pixel x_ef of point i comes from */
enum eds_depth_coords {
    EDS_DEPTH_TRACKS = 0,           /* update(T_kf_ef, kf_coord, tracks) (:137-178): x_ef = x_kf + xy[i] */
    EDS_DEPTH_EF_COORD = 1,         /* update(T_kf_ef, kf_coord, ef_coord) (:101-135): x_ef = xy[i] */
    EDS_DEPTH_REPROJECT = 2,        /* x_ef = x_kf + the track Tracker::getCoord computes at the slot's current pose (Tracker.cpp:343-366,
                                     * eds_trk_update_points' expression in fp64): the whole loop stays on the device; xy unused */
    EDS_DEPTH_DEVICE_TRACKS = 3     /* x_ef = x_kf + the slot's device kf->tracks plane, as the KLT left it (include/eds_hip_klt.h;
                                     * ABI 2): the photometric tracks without a host round trip; xy unused.  EDS_ERR_STATE while the
                                     * handle has no such plane (no eds_klt_track_points* yet) */
};
/* eds::mapping::DEPTH_FILTER (DepthPoints.hpp:31): accepted and ignored, as in the reference (GAUSS runs VOGIATZIS) */
enum eds_depth_filter { EDS_DEPTH_VOGIATZIS = 0, EDS_DEPTH_GAUSS = 1 };
/* per alignment: what one update did */
typedef struct eds_depth_summary {
    int32_t updated;                /* filterVogiatzis ran */
    int32_t skipped_nan;            /* sqrt(sigma2 + tau2) was NaN: seed untouched (DepthPoints.cpp:186-192; zero translation) */
    int32_t sigma2_restored;        /* the new sigma2 was negative: old one kept (:216-220) */
    int32_t mu_reset;               /* mu < 0: mu = 1 (:221-226) */
    int32_t converged;              /* sigma2 < (mu_range / threshold)^2 after the update (isConverged, DepthPoints.hpp:183-193) */
    int32_t pad_;
} eds_depth_summary;
/* DepthPoints::update for slots first .. first + count - 1 in one pass.  Point i of alignment b reads xy[2 * (b * stride + i)]
 * and kf_xy likewise (pixels, N x 2 per alignment, stride >= the largest point count).
 *   kf_xy   NULL: the keyframe pixels the slot holds (fp32 fraction of an integer cell: ~1e-7 px resolution).
 *   xy      NULL only with EDS_DEPTH_REPROJECT and EDS_DEPTH_DEVICE_TRACKS (ignored there).
 *   T_kf_ef count x 7 (p[3], q_xyzw[4]) or NULL: the inverse of each slot's current pose (the tracker's (p, q) is T_ef_kf;
 *           Tracker.cpp:220 hands on its inverse).  EDS_DEPTH_REPROJECT always re-projects at the slot's pose.
 *   filter  an eds_depth_filter, ignored like the reference's.
 *   out     count summaries, or NULL. */
int eds_depth_update(eds_trk* h, int first, int count, int coords, const double* xy, const double* kf_xy, int stride,
                     const double* T_kf_ef, int filter, eds_depth_summary* out);

/* the seeds of a slot, N x 4 (mu, sigma2, a, b) as DepthPoints' vector_type; converged (N, may be NULL): isConverged per point */
int eds_depth_get(eds_trk* h, int slot, double* mu_s2_a_b, uint8_t* converged);
/* operator[] writes (DepthPoints.cpp:264-274): all N seeds of the slot at once; mu goes to the plane as above */
int eds_depth_set(eds_trk* h, int slot, const double* mu_s2_a_b);
/* getIDepth (DepthPoints.cpp:230-246): the fp64 mu of every point, not the fp32 plane */
int eds_depth_get_idepth(eds_trk* h, int slot, double* mu);
/* per alignment of first .. first + count - 1, out4[4 * b ..] = meanIDepth (mean, "std_dev" = the n-1 VARIANCE, 0 for n = 1;
 * Utils.hpp:272-290) and medianIDepth (the nth_element at n/2 and, as "third_q", at n/3; DepthPoints.cpp:255-260) */
int eds_depth_stats(eds_trk* h, int first, int count, double* out4);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_DEPTH_H_ */
