/* eds_hip_kfswitch.h — the keyframe switch of a tracker handle (include/eds_hip.h) for a RANGE of slots without leaving the device:
 * KeyFrame::create (reference src/tracking/KeyFrame.cpp:333-463) for slots first .. first+count-1 in one call, with the depth map of each
 * new keyframe taken from host arrays, from device arrays, or projected on the device from the points another (or the same) slot holds
 * (getDepthMap -> T -> IDepthMap::fromPoints, include/eds_hip_kfpoints.h) — and the depth map's k-d tree built on the device.
 *
 * The tree.  eds_trk_build_keyframe builds the reference's k-d tree (src/utils/KDTree.hpp) on the host with std::nth_element, because an
 * exact distance tie is won by the first point of the tree's traversal and so depends on the tree's shape.  The shape is unique — it
 * does not depend on how nth_element permutes — whenever at every node the median's axis value occurs once among its sub-range: node
 * and sides are then determined as sets, and every position of the index array is the median of some sub-range.  Such a map is built on
 * the device by sorting and partitioning (k_kd_build: one workgroup per map, points and index lists in LDS).  A map is AMBIGUOUS when at
 * some node the median's axis value equals (==: -0.0 equals 0.0) its predecessor's or successor's in the node's axis-sorted list, or when
 * any coordinate is not finite; the kernel detects that exactly, and such a map — or one with more than eds_kfs_tree_capacity() points —
 * is built by the host code eds_trk_build_keyframe uses.  No map is ever built differently from the host: every result of this header
 * equals, bit for bit, what eds_kfp_project_depth_map + eds_trk_build_keyframe give slot by slot.  Projected maps are real-valued and
 * unambiguous except in degenerate poses; integer-pixel maps are the ambiguous ones.
 *
 * Conventions are those of eds_hip_kfpoints.h: plain pointers and sizes, EDS_OK or a negative eds_status, eds_last_error() for the text.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, bad slot ranges, counts, strides or image types, selection parameters
 *    eds_trk_build_keyframe refuses, source and destination ranges that overlap without being equal, a pose or intrinsics that are not
 *    finite, and every device pointer eds_dev_check_range (include/eds_hip_device.h) refuses over the extent that will be read.
 *  - EDS_ERR_STATE: a batch in flight (eds_trk_optimize_batch without eds_trk_sync), a source slot without a keyframe.
 *  Nothing is queued and nothing changes on either of these.  Pointers named d_* are device memory read by kernels; all others are host.
 * A handle that never calls eds_kfs_* allocates and launches nothing of this.  Results have a fixed order: a batch equals its singles bit
 * for bit and runs repeat exactly.  Every call returns when its results are on the host; the slots' Gram matrices follow on the handle's stream, as after eds_dev_set_keyframes.
 */
#ifndef EDS_HIP_KFSWITCH_H_
#define EDS_HIP_KFSWITCH_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_KFSWITCH_ABI_VERSION 1
int eds_kfs_abi_version(void);

/* points per map the device build holds in LDS (4096); larger maps take the host build */
int eds_kfs_tree_capacity(void);
/* slots that eds_kfs_build_keyframes* queues between two waits on the stream */
int eds_kfs_chunk_size(void);

/* The tree alone, for `count` maps in device memory: map b has n[b] >= 0 points (x, y pairs) starting at point b * stride of d_depth_xy
 * (stride >= max n).  perm_out (host, required): at b * stride the n[b] point indices in tree order — node [lo, hi) is position
 * lo + (hi - lo - 1) / 2, its children [lo, mid) and [mid + 1, hi) — exactly edskd::build_tree's array.  on_host_out (host, count bytes,
 * may be NULL): 1 where the map was ambiguous or larger than the capacity and the host build made the array, else 0. */
int eds_kfs_build_tree(eds_trk* h, int count, const int* n, const double* d_depth_xy, int64_t stride, int32_t* perm_out, uint8_t* on_host_out);

typedef enum eds_kfs_depth_source {
    EDS_KFS_DEPTH_NONE = 0,    /* the constant initial depth, as eds_trk_build_keyframe with n_depth = 0 */
    EDS_KFS_DEPTH_HOST = 1,    /* arrays in host memory */
    EDS_KFS_DEPTH_DEVICE = 2,  /* arrays in device memory (range-checked) */
    EDS_KFS_DEPTH_SLOTS = 3    /* the projection of slot src_first + b, as eds_kfp_project_depth_map to the handle's H x W gives it */
} eds_kfs_depth_source;

typedef struct eds_kfs_depth {
    int32_t source;            /* eds_kfs_depth_source */
    int32_t src_first;         /* SLOTS: the first source slot; src_first == first (in place) or the two ranges are disjoint */
    const int* n;              /* HOST / DEVICE: count ints (host), points of map b; 0 = this slot has no map */
    const double* depth_xy;    /* HOST / DEVICE: map b's (x, y) pairs start at point b * stride */
    const double* depth_idp;   /* HOST / DEVICE: ... and its inverse depths */
    int64_t stride;            /* HOST / DEVICE: points between two maps, >= max n */
    const double* T7;          /* SLOTS: count x {p[3], q_xyzw[4]} of T_dst_src, NULL = each source slot's current state */
    const double* K_dst;       /* SLOTS: count x {fx, fy, cx, cy} the map is projected with, NULL = the source slot's own */
} eds_kfs_depth;

/* All host arrays, all optional (NULL).  stride (points between two slots) is needed only with one of the five vectors: >= max_points. */
typedef struct eds_kfs_out {
    int* n_points;             /* count: points kept (what eds_trk_build_keyframe reports) */
    int* status;               /* count: the code eds_trk_build_keyframe would have returned for that slot */
    uint8_t* tree_on_host;     /* count: 1 where the slot's tree came from the host build */
    int64_t stride;
    double* coord_xy;          /* at b * stride: what eds_trk_get_keyframe_points returns after a single build */
    double* norm_xy;
    double* grad_xy;
    double* idp;
    double* weights;
} eds_kfs_out;

/* KeyFrame::create for slots first .. first + count - 1 with one eds_kf_select.  images: count host pointers to grey H x W images of
 * img_type (EDS_IMG_U8 / F32 / F64; resize and RGB stay with eds_trk_build_keyframe_image).  K: count x {fx, fy, cx, cy} of the new
 * keyframes (with EDS_KFS_DEPTH_SLOTS, NULL = each source slot's own).  depth: NULL = EDS_KFS_DEPTH_NONE.  A slot that fails (no candidate, no point above the weight threshold, more points than max_points) is left as it
 * was and the others are still built; the call returns EDS_OK when every slot succeeded, else the first failing slot's code. */
int eds_kfs_build_keyframes(eds_trk* h, int first, int count, int img_type, const void* const* images, const eds_kf_select* sel,
                            const double* K, const eds_kfs_depth* depth, const eds_kfs_out* out);
/* ... with the images in device memory: image b starts at element b * frame_stride of d_images, rows row_stride elements apart
 * (0 = dense: row_stride = W, frame_stride = H * W; otherwise row_stride >= W, frame_stride >= (H - 1) * row_stride + W), aligned to
 * the element size. */
int eds_kfs_build_keyframes_dev(eds_trk* h, int first, int count, int img_type, const void* d_images, int64_t frame_stride,
                                int64_t row_stride, const eds_kf_select* sel, const double* K, const eds_kfs_depth* depth,
                                const eds_kfs_out* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_KFSWITCH_H_ */
