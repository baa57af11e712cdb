/* eds_hip_immature.h — DSO's immature points as EDS uses them on its mapping side, on the device: FrameHessian::makeImages level 0
 * (reference src/tracking/HessianBlocks.cpp:139-202), both ImmaturePoint constructors (src/tracking/ImmaturePoint.cpp:27-114) and
 * ImmaturePoint::traceOn (:128-467) for every point of a range of host frames against the target frame each host names.  The symbols
 * are exported by libeds_hip.so; the object is its own opaque eds_imm, not slots of an eds_trk: host frames and their integer-pixel
 * points are another population than a tracker slot's sub-pixel points, and no entry point of the other headers changes.
 *
 * Conventions are those of eds_hip_kfpoints.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.  Every call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, sizes, ranges, indices or strides out of range, more points than
 *    max_points_per_host, a parameter eds_imm_set_params refuses, a KRKi / Kt / affine pair that is not finite, and every device
 *    pointer eds_dev_check_range (include/eds_hip_device.h) refuses over the extent that will be read: a wrong pointer is an error
 *    code and never a fault.
 *  - EDS_ERR_STATE: eds_imm_create_points on a host frame, eds_imm_trace on a target frame or eds_imm_get_image on a frame that was
 *    never set.  A host without points is traced as what it is: nothing to do, all counts 0.
 *  Nothing is queued and nothing changes on either of these.
 * A process that never calls eds_imm_* allocates and launches nothing of this.  Results have a fixed order and no kernel uses a
 * floating-point atomic: a batch equals its singles bit for bit and runs repeat exactly.
 *
 * Images.  Input is fp32 intensities on DSO's 0 .. 255 scale.  A stored frame is level 0 of makeImages: colour, and dx, dy as halved
 * central differences, a non-finite difference replaced by 0.  The reference's loop runs over the FLAT index W .. W (H - 1) - 1:
 *   dx[i] = 0.5f * (c[i + 1] - c[i - 1]);   dy[i] = 0.5f * (c[i + W] - c[i - W]);
 * so at column 0 and W - 1 the horizontal neighbour is the pixel of the adjacent row, and that is restated here.  Rows 0 and H - 1 are
 * left uninitialised by the reference: here their gradient is 0.  Pyramid levels above 0 and absSquaredGrad are not formed
 * here: only the pixel selector reads absSquaredGrad, and include/eds_hip_select.h forms it.
 *
 * Defined behaviour where the reference reads out of bounds or is undefined.  A sample at (x, y) takes the cell ix = (int)x, iy = (int)y
 * (truncation towards zero, so -1 < x < 0 is cell 0 with a negative fraction, as in the reference) and the 2 x 2 footprint
 * ix .. ix + 1, iy .. iy + 1.  The sample is VALID when x and y are finite with |x|, |y| <= 2^20 and the footprint lies wholly inside the
 * image (0 <= ix <= W - 2, 0 <= iy <= H - 2).  An invalid sample — a rotated pattern tap off the image, a NaN coordinate, the search
 * running a step past uMax — is a non-finite hitColor: the reference's own `energy += 1e5; continue` branch, in the discrete search
 * and in the Gauss-Newton loop alike.  No address is formed from an unchecked coordinate.  A constructor whose pattern has an invalid
 * sample, or a non-finite colour, leaves energyTH = NaN and reports alive = 0 (the reference's caller drops such a point); the point
 * is then ignored by every later call, counted in no summary, and reads back as UNINITIALIZED with the interval [0, NaN].
 * numSteps = (int)(1.9999f + dist / stepsize) is taken as 99 when the float is not below 100.
 *
 * Arithmetic.  Everything is fp32 in the order the reference writes it, without contraction into FMAs, with correctly rounded / and
 * sqrtf.  Where C++ leaves the order to Eigen or to overload resolution it is:
 *   - a matrix-vector product row is summed left to right: pr[i] = (KRKi[i][0] u + KRKi[i][1] v) + KRKi[i][2]; the rotated pattern is
 *     (R00 px + R01 py, R10 px + R11 py);
 *   - the two quadratic forms with gradH are (v^T G) v: t = (vx G00 + vy G10, vx G01 + vy G11), then t0 vx + t1 vy;
 *   - gradH += g g^T per tap in pattern order, entry by entry; squaredNorm is gx gx + gy gy;
 *   - the bilinear weights are dxdy, dy - dxdy, dx - dxdy and ((1 - dx) - dy) + dxdy; the four-term interpolation is ((a + b) + c) + d
 *     in the order (ix+1, iy+1), (ix, iy+1), (ix+1, iy), (ix, iy);
 *   - fabs of a float is the float overload; a double literal that meets a float vector (Kt * 0.01, * 0.5) is narrowed to float first,
 *     as Eigen does; scalar float-with-double-literal expressions (energy += 1e5, step < -0.5) give what their fp32 forms give;
 *   - hw * residual * residual * (2 - hw) is ((hw r) r) (2 - hw); step = ((-gnstepsize) b) / H; errorInPixel = 0.2f + (0.2f (a + b)) / a;
 *   - ptx, pty advance by REPEATED ADDITION of dx, dy, one rounding per step, not i * dx;
 *   - bestIdx is the FIRST index of the minimum (strict < in step order); an energy that is NaN or >= 1e10 is never the best;
 *   - the second constructor forms idepth -+ 0.1 * distance in fp64 and narrows.
 */
#ifndef EDS_HIP_IMMATURE_H_
#define EDS_HIP_IMMATURE_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_IMMATURE_ABI_VERSION 1
int eds_imm_abi_version(void);

typedef struct eds_imm eds_imm;

/* dso::ImmaturePointStatus, in its order */
typedef enum eds_imm_status {
    EDS_IMM_GOOD = 0,
    EDS_IMM_OOB = 1,
    EDS_IMM_OUTLIER = 2,
    EDS_IMM_SKIPPED = 3,
    EDS_IMM_BADCONDITION = 4,
    EDS_IMM_UNINITIALIZED = 5
} eds_imm_status;
#define EDS_IMM_NUM_STATUS 6

/* the setting_* values the constructors and traceOn read (reference src/utils/settings.cpp:90-165) */
typedef struct eds_imm_params {
    float max_pix_search;                 /* setting_maxPixSearch 0.027, relative to W + H */
    float trace_stepsize;                 /* 1 */
    int32_t trace_gn_iterations;          /* 3; 0 .. 16 */
    float trace_gn_threshold;             /* 0.1 */
    float trace_extra_slack_on_th;        /* 1.2 */
    float trace_slack_interval;           /* 1.5 */
    float trace_min_improvement_factor;   /* 2 */
    int32_t min_trace_test_radius;        /* 2; >= 0 */
    float huber_th;                       /* 9 */
    float outlier_th;                     /* 12 * 12 */
    float outlier_th_sum_component;       /* 50 * 50 */
    float overall_energy_th_weight;       /* 1 */
} eds_imm_params;
void eds_imm_params_default(eds_imm_params* p);

/* which = ... of eds_imm_get_image */
#define EDS_IMM_HOST_IMAGE 0
#define EDS_IMM_TARGET_IMAGE 1

/* H, W >= 8; max_hosts, max_points_per_host, max_targets >= 1.  The parameters start as eds_imm_params_default. */
int eds_imm_create(int device, int H, int W, int max_hosts, int max_points_per_host, int max_targets, eds_imm** imm);
void eds_imm_destroy(eds_imm* imm);
/* every float finite; stepsize, max_pix_search, huber_th, outlier_th_sum_component positive; gn_iterations 0 .. 16; radius 0 .. 99 */
int eds_imm_set_params(eds_imm* imm, const eds_imm_params* p);
int eds_imm_get_params(const eds_imm* imm, eds_imm_params* p);

/* Frames first .. first + count - 1: image b starts at element b * frame_stride of `images`, rows row_stride elements apart (0 = dense:
 * row_stride = W, frame_stride = H * W; otherwise row_stride >= W, frame_stride >= (H - 1) * row_stride + W).  on_device = 0: host
 * memory; 1: device memory, range-checked.  Setting a host image leaves that host's points as they are: create them again. */
int eds_imm_set_host_images(eds_imm* imm, int first, int count, const float* images, int64_t frame_stride, int64_t row_stride, int on_device);
int eds_imm_set_target_images(eds_imm* imm, int first, int count, const float* images, int64_t frame_stride, int64_t row_stride, int on_device);

/* Both constructors for the n points of host frame `host`, replacing the points it held: uv n x {u, v} integer pixels, type n floats
 * (my_type, stored only).  idepth and distance both NULL: the first constructor (idepth_min 0, idepth_max NaN, UNINITIALIZED); both
 * given: the second, with its branch on distance > 1.0.  alive_out (n bytes, may be NULL): 0 where the pattern left the image or a
 * colour was not finite.  n = 0 empties the host. */
int eds_imm_create_points(eds_imm* imm, int host, int n, const int32_t* uv, const float* type, const float* idepth, const double* distance,
                          uint8_t* alive_out);
int eds_imm_num_points(const eds_imm* imm, int host, int* n);

/* The first constructor for the pixels an eds_sel (include/eds_hip_select.h) selected, read from the device: the non-zero pixels of its
 * map inside the inclusive rectangle x_min .. x_max, y_min .. y_max, in row-major order, my_type the map value (1, 2 or 4), replacing the
 * points `host` held.  The result equals, bit for bit, eds_imm_create_points called with eds_sel_get_selection's list filtered to the
 * same rectangle.  The rectangle is an argument because the loop that walks the map, FullSystem::makeNewTraces, is not in the reference
 * tree; DSO's own loop runs over patternPadding + 1 <= x < W - patternPadding - 2 with patternPadding = 2, which is x_min = y_min = 3,
 * x_max = W - 5, y_max = H - 5.  n_out (may be NULL): the number of points created; alive_out (may be NULL) takes that many bytes, at
 * the most the n of eds_sel_get_selection.  EDS_ERR_INVALID: imm and sel differ in H, W or device, a rectangle that is not inside the
 * image, more points than max_points_per_host.  EDS_ERR_STATE: no selection yet (eds_sel_make_maps), no host image. */
struct eds_sel;
int eds_imm_create_points_selected(eds_imm* imm, int host, const struct eds_sel* sel, int x_min, int y_min, int x_max, int y_max,
                                   uint8_t* alive_out, int* n_out);

/* traceOn for every live point of hosts first_host .. first_host + count - 1, host first_host + b against target target_index[b] with
 * hostToFrame_KRKi = KRKi[b] (row-major 3 x 3), hostToFrame_Kt = Kt[b], hostToFrame_affine = aff[b].  The same index count times is
 * traceNewCoarse; distinct indices trace a batch.  summary_out (count x EDS_IMM_NUM_STATUS ints, may be NULL): per host the number of
 * live points that hold each status after the call. */
int eds_imm_trace(eds_imm* imm, int first_host, int count, const int32_t* target_index, const float* KRKi, const float* Kt, const float* aff,
                  int32_t* summary_out);

/* per point of `host` (n of eds_imm_num_points; any output may be NULL): lastTraceUV is n x 2 */
int eds_imm_get(eds_imm* imm, int host, float* idepth_min, float* idepth_max, float* quality, int32_t* last_trace_status,
                float* last_trace_uv, float* last_trace_pixel_interval);
/* what the constructor computed: color n x 8, weights n x 8, gradH n x 4 (row-major 2 x 2), energyTH n, alive n bytes */
int eds_imm_get_points(eds_imm* imm, int host, float* color, float* weights, float* gradH, float* energyTH, uint8_t* alive);
/* the stored frame as H x W x {colour, dx, dy}, for tests and debugging */
int eds_imm_get_image(eds_imm* imm, int which, int index, float* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_IMMATURE_H_ */
