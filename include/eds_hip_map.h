/* eds_hip_map.h — the map as EDS publishes it and as the tracker takes it, on the device: the point cloud of the window's active points
 * (dso::io::getMap, reference src/io/OutputMaps.cpp:38-91), of an eds_imm's immature points (getImmatureMap, :93-148) and of a tracker
 * slot's points (KeyFrame::getMap, src/tracking/KeyFrame.cpp:1244-1300), and the IDepthMap2d the next event keyframe is created from:
 * the window's single-point cloud moved into the new keyframe and pushed through IDepthMap::fromPoints (src/mapping/Types.hpp:248-275).
 * This is the one data path from the eds_win of eds_hip_window.h to the eds_trk of eds_hip.h: eds_map_window_depth_maps with
 * on_device = 1 writes exactly the arrays eds_kfs_build_keyframes_dev (eds_hip_kfswitch.h) takes as EDS_KFS_DEPTH_DEVICE, and its n_out is
 * that struct's n.  No per-point array crosses the bus.  The symbols are exported by libeds_hip.so; no entry point of the other headers
 * changes, and a process that never calls eds_map_* allocates and launches nothing new: a handle's scratch is allocated at its first
 * eds_map_* call and freed with the handle.
 *
 * NOT here: PNG and Rock-type output and colour maps; the IMG and EVENTS colour modes of KeyFrame::getMap (a slot holds neither the image
 * nor the model: eds_map_slot_cloud returns points only); the marginalised and outlier point lists (getMap reads only the active
 * pointHessians, and the tables hold only those); IDepthMap::fromDistanceImage / fromDepthmapImage.
 *
 * POSES ARE INPUTS, as everywhere on the DSO side: SE3ToBaseTransform(get_worldToCam_evalPT()).inverse() is the caller's job.  A pose is 12
 * doubles, the rows of [R | t], and must be finite.
 *
 * ARITHMETIC.  getMap mixes widths, and so does this header (csrc/eds_map.hpp is the same code for host and device):
 *   fx, fy, cx, cy are the window's fp32 calibration (getMap narrows hcalib's values to float, :42-45).
 *   a = u - cx, b = v - cy in fp32; for the eight-point fan a = (u - 1) - cx, b = (v + 2) - cy and so on, fp32, left to right (:55-84);
 *   d_i = 1.0 / (double)idepth_scaled (:51);  X = (d_i * (double)a) / (double)fx;  Y = (d_i * (double)b) / (double)fy;  Z = d_i.
 *   A transform is R_i0 X + R_i1 Y + R_i2 Z + t_i, summed left to right in fp64 without contraction — the order eds_hip_kfpoints.h
 *   states.  Eigen's own order inside Transform * Vector3d is not pinned (DESIGN says so); no parity with Eigen is claimed.
 *   Depth maps: the world point is rounded to fp64 and then moved by T_dst_w — two transforms, not one composed matrix; the reference
 *   materialises the world cloud too.  Then px = fx (X' / Z') + cx, py = fy (Y' / Z') + cy, idp' = 1 / Z' (Types.hpp:264), kept iff
 *   px >= 0 && px < dst_W && py >= 0 && py < dst_H (:267), written so that a NaN fails; order preserved.  A point with Z' <= 0 that still
 *   lands in the frame is kept with its non-positive idp', as in eds_hip_kfpoints.h: the reference does not test for it either.
 *   Immature points: d_i = 1.0 / (0.5 * (idepth_max + idepth_min)) (:107), the sum in fp32, the product and the quotient in fp64; a point
 *   with d_i < 0 || !isfinite(d_i) is skipped (:109), and so is a point that is not alive (it is no longer in immaturePoints); order
 *   preserved.  The colour is the reference's table by lastTraceStatus (:112-123): GOOD 0 1 0 1, OOB 1 0 0 1, OUTLIER 0 0 1 1, SKIPPED
 *   0 1 1 1, BADCONDITION 1 1 1 1, UNINITIALIZED 0 0 0 1.
 *   Slot cloud: d = 1.0 / idp;  T_w_kf * (d x_n, d y_n, d) (KeyFrame.cpp:1260-1262), x_n, y_n the slot's stored fp32 normalised
 *   coordinates widened to fp64, idp as eds_kfp_project_depth_map picks it: the seed's fp64 mu when the slot is seeded, else the fp32
 *   inverse-depth plane widened.
 * Every operation is one correctly rounded IEEE operation and there is no floating-point atomic: results have a fixed order, a batch
 * equals its singles bit for bit, runs repeat exactly, and the host restatement edsmap:: gives the same bits.
 *
 * ORDER.  Hosts in window order, each host's points in table order; eight points per point when single_point = 0: the centre, then
 * (0,+2) (-1,+1) (-2,0) (-1,-1) (0,-2) (+1,-1) (+2,0).  The window's points must be grouped by host in nondecreasing host index, as
 * eds_win_accumulate wants them.  Bits of a mask at and above the number of hosts are ignored.
 *
 * Each entry point is one kernel launch and one wait; payloads that stay on the device (on_device = 1) are not copied.  The depth-map
 * kernel runs one workgroup per destination map over the selected hosts' runs in sweeps of 1024 points: a wave64 ballot and a count of
 * the lower lanes give the rank inside a wavefront, the wavefronts' totals are summed from LDS, and a running base goes from sweep to
 * sweep — a stable scatter with no second pass.  The immature cloud is the same compaction by one workgroup.
 *
 * Conventions are those of eds_hip_winedit.h: plain pointers, EDS_OK or a negative eds_status, eds_last_error() for the text.  Every call
 * returns when its counts are on the host and its results are where they were asked for.
 *  - EDS_ERR_INVALID: a NULL handle or required argument; F outside 1 .. 8 or n_hosts outside 1 .. min(32, max_hosts); a point hosted by
 *    a frame at or above F, or hosts that decrease; single_point or on_device that is neither 0 nor 1; a pose, K_dst or calibration
 *    that is not finite; a focal length that is 0 (calib: not positive); count < 1; dst_H or dst_W < 1; a stride smaller than the
 *    points that may be written; a device pointer that eds_dev_check_range (eds_hip_device.h) refuses over the extent that may be read
 *    or written; eds_map_immature_cloud with cap smaller than the cloud — n_out then holds the needed count.
 *  - EDS_ERR_STATE: eds_map_window_* before eds_win_set_calib; eds_map_slot_cloud with a batch in flight or a slot without a keyframe.
 * Nothing is queued and nothing changes on any of these (the too-small cap is found on the device: its kernel writes the count only).
 */
#ifndef EDS_HIP_MAP_H_
#define EDS_HIP_MAP_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"
#include "eds_hip_immature.h"
#include "eds_hip_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_MAP_ABI_VERSION 1
int eds_map_abi_version(void);

#define EDS_MAP_FAN 8                 /* points per map point with single_point = 0 */
#define EDS_MAP_MAX_IMM_HOSTS 32      /* hosts one eds_map_immature_cloud takes */

/* dso::io::getMap for every frame f < F whose bit is set in frame_mask.  T_w_c: F x 12, host memory.  points: n_out x 3 doubles, host
 * memory, or the caller's device memory with on_device = 1; n_out = (single_point ? 1 : 8) x the selected hosts' points, known before
 * the launch (points may be NULL when it is 0).  per_host (may be NULL): [8] the selected points per host, 0 for the others. */
int eds_map_window_cloud(eds_win* win, int F, uint32_t frame_mask, const double* T_w_c, int single_point, double* points, int on_device,
                         int32_t* n_out, int32_t* per_host);

/* The single-point cloud, each world point moved by T_dst_w[b] (count x 12, host memory) and pushed through IDepthMap::fromPoints with
 * K_dst[b] (count x 4: fx, fy, cx, cy) and {dst_W, dst_H}.  Map b starts at point b * stride of depth_xy (x 2), depth_idp and src_index
 * (may be NULL; the point's index in the window's table): the layout of eds_kfs_depth with EDS_KFS_DEPTH_HOST, or with on_device = 1
 * EDS_KFS_DEPTH_DEVICE; n_out[b] (count entries, host memory) is that struct's n.  stride >= the selected hosts' points. */
int eds_map_window_depth_maps(eds_win* win, int F, uint32_t frame_mask, const double* T_w_c, int count, const double* T_dst_w,
                              const double* K_dst, int dst_H, int dst_W, int64_t stride, double* depth_xy, double* depth_idp,
                              int32_t* src_index, int on_device, int32_t* n_out);

/* getImmatureMap for hosts h < n_hosts whose bit is set in host_mask.  T_w_c: n_hosts x 12; calib: fx, fy, cx, cy as getImmatureMap
 * narrows them.  points (x 3), colors (x 4 doubles, may be NULL) and status (the lastTraceStatus code itself, may be NULL) hold cap
 * entries each; n_out: the entries written.  cap too small: EDS_ERR_INVALID, n_out holds the needed count, the outputs are untouched. */
int eds_map_immature_cloud(eds_imm* imm, int n_hosts, uint32_t host_mask, const double* T_w_c, const float calib[4], int single_point,
                           int64_t cap, double* points, double* colors, uint8_t* status, int on_device, int32_t* n_out);

/* A host's trace results replaced from host memory (n = eds_imm_num_points entries each; any pointer may be NULL: that column stays):
 * what a caller that keeps immature points elsewhere, and a test of eds_map_immature_cloud, put in front of it.  Nothing else of the
 * points changes. */
int eds_map_set_immature_trace(eds_imm* imm, int host, const float* idepth_min, const float* idepth_max, const int32_t* last_trace_status);

/* KeyFrame::getMap's points of tracker slots first .. first + count - 1.  T_w_kf: count x 12.  Slot b's N points are at b * stride of
 * points (x 3; host memory, or device memory with on_device = 1), n_out[b] = N.  stride >= the largest N. */
int eds_map_slot_cloud(eds_trk* h, int first, int count, const double* T_w_kf, int stride, double* points, int on_device, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_MAP_H_ */
