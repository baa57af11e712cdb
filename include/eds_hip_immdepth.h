/* eds_hip_immdepth.h — a keyframe's immature points seeded from a depth map that lives on the device.  EDS does not create a new keyframe's
 * immature points blind: ImmaturePoint's second constructor (reference src/tracking/ImmaturePoint.cpp:68-114) takes the inverse depth of
 * the nearest depth-map point and the distance to it, and within one pixel the point starts IPS_GOOD with the interval
 * idepth -+ 0.1 distance.  Here the map (the layout eds_map_window_depth_maps of eds_hip_map.h writes for one map), its k-d tree, the
 * selector's pixel list (eds_hip_select.h), the nearest-neighbour walk and the constructor all stay on the device: a keyframe cycle runs
 * selection -> seeded immature points -> trace -> activation -> window -> map -> next keyframe, and no per-point or per-pixel array
 * crosses the bus in either direction.  The symbols are exported by libeds_hip.so; the state hangs off the eds_imm of
 * eds_hip_immature.h, is allocated by the first eds_imd_* call and freed by eds_imm_destroy; a process that never calls eds_imd_*
 * allocates and launches nothing new, and no entry point of the other headers changes.
 *
 * THE LOOP.  The loop that drives the constructor is not in the reference tree (it lives in the external component); it is stated here,
 * modelled on the one in-tree use of the tree, KeyFrame::setDepthMap (src/tracking/KeyFrame.cpp:1151-1163).  For each created pixel
 * (u, v), in list order:
 *   1. q = (u * scale[0], v * scale[1]) in fp64;
 *   2. k = KDTree::nnSearch(q) exactly as eds_hip_kfswitch.h pins it: a guess is replaced only on a strict <, the near side is walked
 *      first, and an exact tie goes to the first point of the traversal;
 *   3. idepth = (float)map.idepth[k];
 *   4. distance = sqrt(dx * dx + dy * dy), dx = map.x[k] - u, dy = map.y[k] - v against the UNSCALED pixel, in fp64, every product
 *      and the sum rounded on its own (no FMA);
 *   5. the second constructor, with its branch on distance > 1.0 (a distance of exactly 1.0 is GOOD; a NaN distance is GOOD too, as
 *      `!(distance > 1.0)` is what the reference's else branch takes).
 * An empty map (n = 0) is the first constructor for every pixel: bit for bit eds_imm_create_points_selected / eds_imm_create_points
 * without idepth.  Inverse depths are carried as they are: a negative or NaN inverse depth at the winner reaches the point unchanged.
 * After a create call the points are ordinary eds_imm points: eds_imm_trace, eds_act_*, eds_map_immature_cloud and eds_imm_get* see no
 * difference from points made by eds_imm_create_points(idepth, distance) with the same values.
 *
 * THE TREE.  Maps of up to eds_kfs_tree_capacity() points are built on the device by the kernel of eds_hip_kfswitch.h on the eds_imm's
 * own stream; a map that is ambiguous (eds_hip_kfswitch.h), or larger, is downloaded and built by the host's std::nth_element build,
 * exactly as eds_kfs_build_tree does it.  Both give the same array.  The map then stays on the device in tree order until the next
 * eds_imd_set_depth_map.
 *
 * WAITS.  A create call is queued without a host wait in between — rectangle filter, nearest neighbour, constructor, the kernels
 * reading the count on the device — and then waits ONCE, for the count, the alive bytes and the two status counts.  eds_imd_info.waits
 * counts the waits of the last create call.
 *
 * Conventions are those of eds_hip_immature.h: plain pointers, EDS_OK or a negative eds_status, eds_last_error() for the text, and
 * nothing changed on an error: the handle's points, its map and what eds_imd_get_nearest returns stay as they were.
 *  - EDS_ERR_INVALID: a NULL handle or required argument; n < 0; on_device neither 0 nor 1; a map coordinate that is not finite; a
 *    scale that is not finite; a selector of another size or device; a rectangle that is not inside the image; more pixels than
 *    max_points_per_host; a device pointer eds_dev_check_range (eds_hip_device.h) refuses over the extent that will be read, or one that
 *    is not aligned to its element.
 *  - EDS_ERR_STATE: a create call before eds_imd_set_depth_map; a host frame without an image; a selector without a selection (never
 *    made, or made stale by a new image or new parameters); eds_imd_get_nearest on a host no eds_imd_create_* call has filled.
 */
#ifndef EDS_HIP_IMMDEPTH_H_
#define EDS_HIP_IMMDEPTH_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"
#include "eds_hip_immature.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_IMMDEPTH_ABI_VERSION 1
int eds_imd_abi_version(void);

/* how the nearest-neighbour pass walked the tree: the one form the library has */
#define EDS_IMD_WALK_GLOBAL 1 /* the tree in global memory, each lane's pending sides in private memory */

typedef struct eds_imd_info {
    int32_t map_set;      /* 1 after a successful eds_imd_set_depth_map */
    int32_t map_n;        /* its points */
    int32_t tree_on_host; /* 1: the host built its tree */
    int32_t waits;        /* host waits of the last eds_imd_create_* call */
    int32_t walk;         /* the form its nearest-neighbour pass took (EDS_IMD_WALK_GLOBAL; 0: no pass, the map was empty) */
    int32_t reserved;
    float nn_kernel_ms;   /* with timing on: the nearest-neighbour pass alone, and ... */
    float queue_ms;       /* ... everything the call queued, first kernel to last copy; 0 otherwise */
} eds_imd_info;

/* The depth map the next create calls seed from: n >= 0 points, depth_xy n x {x, y} and depth_idp n doubles, in host memory
 * (on_device = 0) or device memory (1, range-checked).  tree_on_host (may be NULL): 0 the device built the tree, 1 the host did. */
int eds_imd_set_depth_map(eds_imm* imm, int n, const double* depth_xy, const double* depth_idp, int on_device, int* tree_on_host);

/* The loop above for the pixels an eds_sel selected: the non-zero pixels of its map inside the inclusive rectangle, in row-major order,
 * my_type the map value, replacing the points `host` held — eds_imm_create_points_selected's checks, order and overflow behaviour.
 * scale: 2 doubles, NULL = {1, 1}.  n_out (may be NULL): the points created; alive_out (may be NULL) takes that many bytes, at the most
 * min(the n of eds_sel_get_selection, max_points_per_host); status_counts_out (may be NULL): [2], the alive points that start GOOD and
 * UNINITIALIZED. */
struct eds_sel;
int eds_imd_create_points_selected(eds_imm* imm, int host, const struct eds_sel* sel, int x_min, int y_min, int x_max, int y_max,
                                   const double* scale, uint8_t* alive_out, int* n_out, int32_t* status_counts_out);

/* The same for a caller's own list: uv n x {u, v} integer pixels and type n floats, both in host memory (on_device = 0) or both in
 * device memory (1, range-checked).  n = 0 empties the host. */
int eds_imd_create_points(eds_imm* imm, int host, int n, const int32_t* uv, const float* type, int on_device, const double* scale,
                          uint8_t* alive_out, int32_t* status_counts_out);

/* Per point of the last eds_imd_create_* on `host` (n of eds_imm_num_points entries; any output may be NULL): the winner's index in the
 * caller's map order, the narrowed inverse depth and the fp64 distance; -1, 0 and 0 where the map was empty.  For tests and debugging. */
int eds_imd_get_nearest(eds_imm* imm, int host, int32_t* index_out, float* idepth_out, double* distance_out);

/* The map in tree order: perm (position -> the caller's index), txy (x 2) and tidp, map_n entries each; any may be NULL.  For tests. */
int eds_imd_get_tree(eds_imm* imm, int32_t* perm_out, double* txy_out, double* tidp_out);

/* For measurements: whether the next create calls time their kernels with events (0 / 1).  eds_imd_get_info reads the record above. */
int eds_imd_set_debug(eds_imm* imm, int timing);
int eds_imd_get_info(eds_imm* imm, eds_imd_info* info);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_IMMDEPTH_H_ */
