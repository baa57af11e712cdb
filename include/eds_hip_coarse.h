/* eds_hip_coarse.h — DSO's coarse image tracker as EDS uses it for the pose of every new image frame, on the device:
 * dso::CoarseTracker (reference src/tracking/CoarseTracker.cpp:93-701) with every level of FrameHessian::makeImages
 * (src/tracking/HessianBlocks.cpp:139-202).  It aligns the new image to the last keyframe, image to image, coarse to fine, over 8
 * parameters: SE(3) and the affine brightness pair (a, b).  The symbols are exported by libeds_hip.so; the object is its own opaque
 * eds_ct with a pyramid of its own (eds_imm's images are another object and do not change), and no entry point of the other headers
 * changes.
 *
 * Conventions are those of eds_hip_immature.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.  Every call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, sizes, levels or strides out of range, a shape eds_ct_create refuses, a
 *    parameter eds_ct_set_params refuses, a pose, affine pair, exposure, cutoff or calibration that is not finite, and every device
 *    pointer eds_dev_check_range (include/eds_hip_device.h) refuses over the extent that will be read: a wrong pointer is an error
 *    code and never a fault.
 *  - EDS_ERR_STATE: eds_ct_set_ref before eds_ct_set_calib; eds_ct_track or eds_ct_calc_res before the calibration and both frames
 *    are set; eds_ct_get_level of a frame that was never set.
 *  Nothing is queued and nothing changes on either of these.
 * A process that never calls eds_ct_* allocates and launches nothing of this.  No kernel uses a floating-point atomic and every
 * result has a fixed order: a batch of tries equals its singles bit for bit and runs repeat exactly.
 *
 * What is restated, with the reference's lines.
 *  1. makeK (:93-122).  w >> l, h >> l; fx_l = fx_{l-1} * 0.5; cx_l = (cx_0 + 0.5) / 2^l - 0.5, formed in fp64 from the fp32 operands
 *     and narrowed to the fp32 member, as the C++ does.  Ki is the CLOSED FORM fxi = 1 / fx, cxi = -cx / fx (fp32), not Eigen's 3 x 3
 *     inverse.  H and W must be divisible by 2^(levels - 1) and the coarsest level be at least 8 x 8.
 *  2. makeImages, all levels (HessianBlocks.cpp:139-202).  Colour of level l is 0.25f * (((a + b) + c) + d) over (2x, 2y), (2x + 1, 2y),
 *     (2x, 2y + 1), (2x + 1, 2y + 1); dx, dy at every level follow the FLAT-index rule eds_hip_immature.h documents for level 0 (at
 *     column 0 and w - 1 the horizontal neighbour is the pixel of the adjacent row); a non-finite difference is 0; rows 0 and h - 1
 *     have gradient 0.  absSquaredGrad is not formed here (eds_hip_select.h forms it).  Level 0 equals eds_imm_get_image of the same frame bit for bit.
 *  3. setCoarseTrackingRef / makeCoarseDepthL0 (:126-283).  The caller passes, per active residual, centerProjectedTo (n x 3 floats)
 *     and HdiF (n floats).  u = (int)(x + 0.5f), truncating towards zero; weight = sqrtf((float)(1e-3 / (HdiF + 1e-12))) with the sum and
 *     the quotient in fp64.  A contribution whose x + 0.5f or y + 0.5f is not finite, <= -1 or >= W (H) is DROPPED and counted (the
 *     reference would write out of bounds).  idepth[0] / weightSums[0] equal the serial loop in input order bit for bit: the device
 *     records per pixel, with integer atomics, the smallest and largest input index; a lone contribution is written as 0 + x, and for
 *     any other pixel the thread of the smallest index walks the inputs up to the largest and adds those of its pixel in index order.
 *     Level sums are ((a + b) + c) + d in the reference's tap order; the dilation (diagonal at levels 0 and 1, the cross above) reads
 *     the undilated planes and writes only where the weight is <= 0; a neighbour index outside the plane — the reference reads one
 *     element before and one after it — counts as empty.  The normalisation runs over 2 <= x < w - 2, 2 <= y < h - 2 and, as the
 *     reference's `continue` does, leaves weightSums untouched where the colour is not finite or the idepth not > 0.  The pc_* lists
 *     come out in ROW-MAJOR order by a stable compaction (ballot, block scan, counts of the workgroups before).
 *  4. calcRes (:349-498), every branch.  RKi = R.cast<float>() * Ki with every coefficient summed left to right, Ki's zeros included;
 *     t and the affine pair (AffLight::fromToVecExposure, NumType.h:175-187, in fp64) are narrowed to float; pt = (RKi (x, y, 1)) + t id
 *     with the product row summed left to right.  The lvl == 0 && i % 32 == 0 flow terms are restated.  The bounds test is
 *     Ku > 2 && Kv > 2 && Ku < wl - 3 && Kv < hl - 3 && new_idepth > 0; a NaN fails it, so no address is formed from an unchecked
 *     coordinate.  getInterpolatedElement33 has the weights dxdy, dy - dxdy, dx - dxdy and ((1 - dx) - dy) + dxdy and sums
 *     ((w11 v11 + w01 v01) + w10 v10) + w00 v00 in the order (ix+1, iy+1), (ix, iy+1), (ix+1, iy), (ix, iy).  The Huber weight is
 *     |r| < huberTH ? 1 : huberTH / |r|; a term with |r| > cutoff adds maxEnergy = (2 huberTH) cutoff - huberTH huberTH and is
 *     saturated; any other adds ((hw r) r) (2 - hw) and writes its buf_warped_* row.
 *  5. calcGSSSE (:287-344).  The eight Jacobian entries and the residual as the _mm_* calls nest them; each of the 45 terms is
 *     (J_a w) J_b with two fp32 roundings; a and b0 are narrowed to float; the division is by the PADDED count (n rounded up to a
 *     multiple of 4) as (double)(1.0f / n); the SCALE_* factors (HessianBlocks.h:58-65) multiply columns, then rows.  n == 0 gives a
 *     non-finite H; the loop's isfinite test then zeroes the step.
 *  6. trackNewestCoarse (:520-701), whole: the cutoff doubling, lambda = 0.01, the extrapolation factor, the four affineOptMode
 *     cases of the solve, SE3::exp(inc) * T (sophus/se3.hpp:406-428), the accept test, lambda *= 0.5 or 4, the inc.norm() > 1e-3 break,
 *     lastResiduals and lastFlowIndicators, the minResForAbort return (pose and affine pair then stay the inputs, as in the reference),
 *     the single level repeat, the final affine checks and the zeroing of a fixed a / b.
 *
 * Sums.  The reference adds E and Accumulator9's 45 entries in fp32 in serial order (three tiers); no parallel code has that rounding.
 * Here every per-point TERM is the reference's fp32 value; the terms are widened to fp64 and added in the one fixed order
 * csrc/eds_coarse.hpp defines (512 lanes striding the list, a fold inside every 64 lanes, the eight totals left to right); the counts
 * are integers.  The host restatement edsct::track_serial walks the same order, so it and the device agree bit for bit on rs, H, b and
 * every row, and both agree with the fp32-summing reference to its own rounding error.  fp64 sin, cos and exp are the header's own
 * plain-arithmetic edsct::sincos_d / exp_d (within 2 ulps and 1 ulp of libm over every argument they accept), the solves an unpivoted
 * L D L^T written out there (Eigen's pivoted ldlt() is not restated), the pose a 3 x 4 matrix [R | t] updated as Rinc R, Rinc t + V u
 * (Sophus keeps a quaternion), and fabsf(logf(x)) > 1.5 of the last check is x > e^1.5 or 0 <= x < e^-1.5 — so the pose, the affine
 * pair, the iteration counts, the accept sequence and lastResiduals of the host restatement and the device are identical.
 */
#ifndef EDS_HIP_COARSE_H_
#define EDS_HIP_COARSE_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_COARSE_ABI_VERSION 1
int eds_ct_abi_version(void);

typedef struct eds_ct eds_ct;

#define EDS_CT_MAX_LEVELS 5
#define EDS_CT_MAX_DECISIONS 512
/* the most contributions of one eds_ct_set_ref: the order-exact scatter walks, per colliding pixel, the inputs between its first and
 * last contribution, at the worst n^2 / 2 steps in one launch, and this keeps that worst case to a fraction of a second */
#define EDS_CT_MAX_POINTS 65536

/* the setting_* values trackNewestCoarse reads (reference src/utils/settings.cpp:119-138) */
typedef struct eds_ct_params {
    float huber_th;                       /* setting_huberTH 9 */
    float coarse_cutoff_th;               /* setting_coarseCutoffTH 20 */
    float affine_opt_mode_a;              /* setting_affineOptModeA 1e12; < 0: a is fixed */
    float affine_opt_mode_b;              /* setting_affineOptModeB 1e8; < 0: b is fixed */
} eds_ct_params;
void eds_ct_params_default(eds_ct_params* p);

/* one try of eds_ct_track */
typedef struct eds_ct_result {
    double T[12];                         /* lastToNew_out, row-major 3 x 4 [R | t] */
    double aff[2];                        /* aff_g2l_out (a, b) */
    double last_residuals[5];             /* lastResiduals; NaN for a level that was not reached */
    double last_flow_indicators[3];
    int32_t ok;                           /* the bool trackNewestCoarse returns */
    int32_t n_decisions;
    int32_t iterations[EDS_CT_MAX_LEVELS];        /* per level, a repeated level included */
    int32_t accepts[EDS_CT_MAX_LEVELS];
    float level_cutoff_repeat;            /* of the last level that ran */
    int32_t reserved;
    uint8_t decisions[EDS_CT_MAX_DECISIONS];      /* per iteration, in order: bit 0 accept, bits 1 .. the level */
} eds_ct_result;

/* one list entry of eds_ct_calc_res, 16 words: in_e and not warped is a saturated term; the buf_warped_* row is valid when warped, the
 * four flow addends (translation +, translation -, rotation and translation +, -) when flow */
typedef struct eds_ct_row {
    int32_t in_e, warped, flow;
    float energy;
    float idepth, u, v, dx, dy, residual, weight, ref_color;
    float shift_t_pos, shift_t_neg, shift_rt_pos, shift_rt_neg;
} eds_ct_row;

/* which = ... of eds_ct_get_level */
#define EDS_CT_REF_IMAGE 0                /* h x w x {colour, dx, dy} */
#define EDS_CT_NEW_IMAGE 1
#define EDS_CT_IDEPTH 2                   /* h x w, after dilation and normalisation */
#define EDS_CT_WEIGHT_SUMS 3
#define EDS_CT_PC 4                       /* pc_n x {u, v, idepth, colour} */

/* levels 1 .. 5; H, W 8 .. 8192, divisible by 2^(levels - 1), the coarsest level at least 8 x 8; max_points 1 .. EDS_CT_MAX_POINTS contributions
 * per eds_ct_set_ref; max_tries >= 1 per eds_ct_track.  The parameters start as eds_ct_params_default. */
int eds_ct_create(int device, int H, int W, int levels, int max_points, int max_tries, eds_ct** ct);
void eds_ct_destroy(eds_ct* ct);
/* every float finite; huber_th and coarse_cutoff_th positive */
int eds_ct_set_params(eds_ct* ct, const eds_ct_params* p);
int eds_ct_get_params(const eds_ct* ct, eds_ct_params* p);
/* level-0 intrinsics: finite, fx and fy positive */
int eds_ct_set_calib(eds_ct* ct, float fx, float fy, float cx, float cy);
/* K = {fx, fy, cx, cy} of level lvl */
int eds_ct_get_k(const eds_ct* ct, int lvl, float* K);

/* The reference frame: its image (fp32, DSO's 0 .. 255 scale; rows row_stride elements apart, 0 = W; on_device = 1: device memory,
 * range-checked), ab_exposure and aff_g2l, and the n contributions in the window optimiser's order.  pc_n_out (levels ints, may be
 * NULL): the list sizes; dropped_out (may be NULL): contributions outside the image. */
int eds_ct_set_ref(eds_ct* ct, const float* image, int64_t row_stride, int on_device, float exposure, double aff_a, double aff_b, int n,
                   const float* center_projected, const float* hdif, int32_t* pc_n_out, int32_t* dropped_out);
int eds_ct_set_new(eds_ct* ct, const float* image, int64_t row_stride, int on_device, float exposure);

/* trackNewestCoarse for `count` initial guesses (T_init count x 12, aff_init count x 2) against the frames the object holds, one
 * workgroup each; min_res_for_abort has 5 entries.  results: count entries. */
int eds_ct_track(eds_ct* ct, int count, const double* T_init, const double* aff_init, int coarsest_lvl, const double* min_res_for_abort,
                 eds_ct_result* results);

/* calcRes and calcGSSSE once, by the device code eds_ct_track runs: rs_out 6, H_out 64 (row-major 8 x 8), b_out 8, rows_out one entry
 * per list entry of the level (any output may be NULL) */
int eds_ct_calc_res(eds_ct* ct, int lvl, const double* T, const double* aff, float cutoff, double* rs_out, double* H_out, double* b_out,
                    eds_ct_row* rows_out);

/* one level of what the object holds, for tests and debugging; out must hold h x w x 3, h x w, or (EDS_CT_PC) 4 floats per list entry;
 * n_out (may be NULL): the pixels or list entries written */
int eds_ct_get_level(eds_ct* ct, int which, int lvl, float* out, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_COARSE_H_ */
