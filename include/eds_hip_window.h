/* eds_hip_window.h — the per-residual and per-point part of DSO's window optimiser on the device: PointFrameResidual::linearize over
 * every residual of the window (reference src/tracking/Residuals.cpp:69-265), applyRes with EFResidual::takeDataF (Residuals.cpp:298-320,
 * src/bundles/EnergyFunctionalStructs.cpp:38-48), the per-point sums of AccumulatedTopHessianSSE::addPoint<0>
 * (src/bundles/AccumulatedTopHessian.cpp:49-145) and the per-point prologue of AccumulatedSCHessianSSE::addPoint
 * (src/bundles/AccumulatedSCHessian.cpp:36-55).  It reads level 0 of FrameHessian::makeImages and the color[8] / weights[8] that
 * eds_imm_create_points produces; it writes centerProjectedTo and HdiF, the two inputs eds_ct_set_ref asks its caller for.  The symbols
 * are exported by libeds_hip.so; the object is its own opaque eds_win, and no entry point of the other headers changes.
 *
 * eds_win_accumulate adds every accumulator of the two addPoint()s (acc[h + F t], accHcc, accbc, accD, accE, accEB) on the device and
 * both stitches (in fp64, one thread per output entry, the addends in the header's order) and returns H_A, b_A, H_sc, b_sc.
 * NOT here: modes 1 and 2 of the top accumulator, point marginalisation, the priors of usePrior (a diagonal add), the dense solve and
 * resubstituteF are eds_hip_winsolve.h's, over this object.  Without that header no residual carries isLinearized: such residuals must
 * then stay out of the table, and their sums come in through lf (lf = NULL: the sums eds_hip_winsolve.h left on the device, if any).
 *
 * Conventions are those of eds_hip_coarse.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.  Every call returns when its results are on the device or the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, sizes, frames or strides out of range, a parameter eds_win_set_params
 *    refuses, a calibration, precalc record or threshold that is not finite, a residual whose target is its host, residuals that are
 *    not grouped by point in nondecreasing point index, points that are not grouped by host frame, and every device pointer
 *    eds_dev_check_range (include/eds_hip_device.h) refuses over the extent that will be read.
 *  - EDS_ERR_STATE: eds_win_linearize before the calibration and frames 0 .. F - 1 are set; eds_win_apply before a linearize.
 *  Nothing is queued and nothing changes on either of these.
 * No kernel uses a floating-point atomic and every result has a fixed order: runs repeat exactly.
 *
 * What is restated, with the reference's lines.
 *  1. Level 0 of makeImages (HessianBlocks.cpp:139-202): one pixel is {colour, dx, dy}, by the code of eds_hip_coarse.h (its item 2);
 *     a frame equals eds_ct_get_level(.., 0) and eds_imm_get_image of the same image bit for bit.
 *  2. Both projectPoint overloads (ResidualProjections.h:46-86).  Every row of R * KliP and KRKi * (u, v, 1) is summed left to right,
 *     then the translation's term is added.  The bounds are Ku > 1.1f && Kv > 1.1f && Ku < W - 3 && Kv < H - 3, written so that a NaN
 *     fails; the long overload tests drescale > 0 first.  No address is formed before the test passes.
 *  3. linearize, whole (Residuals.cpp:69-265).  Jpdxi, Jpdc, Jpdd with SCALE_IDEPTH, SCALE_F, SCALE_C and every product in the
 *     reference's left-to-right order; the 8 taps of staticPattern[8] = (0,-2) (-1,-1) (1,-1) (-2,0) (0,0) (2,0) (-1,1) (0,2);
 *     getInterpolatedElement33 as ((dxdy v11 + (dy - dxdy) v01) + (dx - dxdy) v10) + (((1 - dx) - dy) + dxdy) v00;
 *     w = 0.5f (sqrtf(c / (c + (dx dx + dy dy))) + weights[idx]); the Huber weight and its sqrtf; energyLeft += ((((w w) hw) r) r) (2 - hw);
 *     the ten fp32 running sums and wJI2_sum added in pattern order 0 .. 7; JabF zeroed where affineOptModeA / B < 0; the outlier rule
 *     energy > max(frameEnergyTH host, target) || wJI2_sum < 2.  A residual that ends OOB keeps EVERY word of its J from the previous
 *     linearize (the reference leaves it half-written; nothing reads it); centerProjectedTo and the projectedTo entries are written
 *     exactly as far as the reference's loop had written them.
 *  4. applyRes(copyJacobians) and takeDataF: state, energy, isActiveAndIsGoodNEW, the functional's J (a copy where the reference swaps two
 *     pointers) and JpJdF.
 *  5. Per point, residuals in table order: JI_r, Hdd_accAF, bd_accAF, Hcd_accAF, nres; then the ngoodres == 0 branch, the H < 1e-10 clamp,
 *     idepth_hessian, HdiF = (float)(1.0 / H), bdSumF (with shiftPriorToZero).  priorF, deltaF and the linearized sums are inputs.
 * The energy eds_win_linearize returns is the fp64 sum of the per-residual fp32 returns in the order csrc/eds_window.hpp names (512 lanes
 * striding the residual index, a fold inside every 64, the eight totals left to right).  The host restatement edswin::linearize_serial
 * walks the same order, so it and the device agree bit for bit on every output.
 */
#ifndef EDS_HIP_WINDOW_H_
#define EDS_HIP_WINDOW_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_WINDOW_ABI_VERSION 1
int eds_win_abi_version(void);

typedef struct eds_win eds_win;

#define EDS_WIN_MAX_FRAMES 8
/* one FrameFramePrecalc as linearize reads it (HessianBlocks.cpp:204-234), matrices row-major:
 * PRE_KRKiTll[9], PRE_KtTll[3], PRE_RTll_0[9], PRE_tTll_0[3], PRE_aff_mode[2], PRE_b0_mode */
#define EDS_WIN_PRECALC_FLOATS 27
/* one RawResidualJacobian, 2 x 2 blocks row-major: resF[8], Jpdxi[2][6], Jpdc[2][4], Jpdd[2], JIdx[2][8], JabF[2][8], JIdx2[2][2],
 * JabJIdx[2][2], Jab2[2][2] */
#define EDS_WIN_J_WORDS 74
/* ResState (Residuals.h:47) */
#define EDS_WIN_IN 0
#define EDS_WIN_OOB 1
#define EDS_WIN_OUTLIER 2

/* the setting_* values and SCALE_* constants linearize reads (reference src/utils/settings.cpp:91-127, HessianBlocks.h:58-62) */
typedef struct eds_win_params {
    float outlier_th_sum_component;       /* setting_outlierTHSumComponent 50 * 50 */
    float huber_th;                       /* setting_huberTH 9 */
    float affine_opt_mode_a;              /* setting_affineOptModeA 1e12; < 0: JabF[0] is zeroed */
    float affine_opt_mode_b;              /* setting_affineOptModeB 1e8; < 0: JabF[1] is zeroed */
    float scale_idepth;                   /* SCALE_IDEPTH 1 */
    float scale_f;                        /* SCALE_F 1 */
    float scale_c;                        /* SCALE_C 1 */
    float reserved;
} eds_win_params;
void eds_win_params_default(eds_win_params* p);

/* the outputs of eds_win_get_residuals, one entry per residual in table order; any pointer may be NULL */
typedef struct eds_win_residual_out {
    int32_t* state;                       /* state_state */
    float* energy;                        /* state_energy */
    int32_t* new_state;                   /* state_NewState */
    float* new_energy;                    /* state_NewEnergy */
    float* new_energy_with_outlier;       /* state_NewEnergyWithOutlier */
    float* linearize_return;              /* what the last linearize returned for the residual */
    int32_t* is_active;                   /* efResidual->isActiveAndIsGoodNEW */
    float* center_projected_to;           /* x 3 */
    float* projected_to;                  /* x 8 x 2 */
    float* J;                             /* x EDS_WIN_J_WORDS: the residual's own, what linearize wrote */
    float* ef_J;                          /* x EDS_WIN_J_WORDS: the energy functional's, what takeDataF left */
    float* JpJdF;                         /* x 8 */
} eds_win_residual_out;

/* the outputs of eds_win_get_points, one entry per point; any pointer may be NULL */
typedef struct eds_win_point_out {
    float* Hdd_accAF;
    float* bd_accAF;
    float* Hcd_accAF;                     /* x 4 */
    float* HdiF;
    float* bdSumF;
    float* idepth_hessian;
    int32_t* nres;                        /* the point's active residuals */
} eds_win_point_out;

/* H, W 8 .. 8192; max_frames 2 .. EDS_WIN_MAX_FRAMES; max_points >= 1, max_residuals >= 1.  The parameters start as eds_win_params_default. */
int eds_win_create(int device, int H, int W, int max_frames, int max_points, int max_residuals, eds_win** win);
void eds_win_destroy(eds_win* win);
/* every float finite; outlier_th_sum_component, huber_th and the three scales positive */
int eds_win_set_params(eds_win* win, const eds_win_params* p);
int eds_win_get_params(const eds_win* win, eds_win_params* p);
/* HCalib's fxl, fyl, cxl, cyl: finite, fx and fy positive; fxli = 1 / fxl as CalibHessian forms it */
int eds_win_set_calib(eds_win* win, float fx, float fy, float cx, float cy);

/* frames first .. first + count - 1 of the window: fp32 images on DSO's 0 .. 255 scale, rows row_stride elements apart (0 = W), frames
 * frame_stride elements apart (0 = H * row_stride); on_device = 1: device memory, range-checked */
int eds_win_set_frames(eds_win* win, int first, int count, const float* images, int64_t row_stride, int64_t frame_stride, int on_device);
/* one frame as H x W x {colour, dx, dy} */
int eds_win_get_frame(eds_win* win, int frame, float* out);

/* the window's points, grouped by host frame: host[n], uv[n][2], color[n][8], weights[n][8], idepth_scaled[n], idepth_zero_scaled[n].
 * The residual table becomes empty, on the device as well: every point's run is [0, 0) and nothing is active. */
int eds_win_set_points(eds_win* win, int n, const int32_t* host, const float* uv, const float* color, const float* weights,
                       const float* idepth_scaled, const float* idepth_zero_scaled);
/* per iteration, after a step; either pointer may be NULL (that value stays) */
int eds_win_set_idepths(eds_win* win, const float* idepth_scaled, const float* idepth_zero_scaled);
/* the residuals, grouped by point in nondecreasing point index (a point's run is its residualsAll): point[m], target[m], state[m] (NULL:
 * all IN), energy[m] (NULL: 0).  As resetOOB leaves them: state_NewState = OUTLIER, state_NewEnergy = state_energy, not active, J zero. */
int eds_win_set_residuals(eds_win* win, int m, const int32_t* point, const int32_t* target, const int32_t* state, const float* energy);

/* linearize for every residual: precalc[(host * F + target) * 27] (the diagonal is not read but must be finite), frame_energy_th[F].
 * energy (may be NULL): the sum of the returns; counts (3 ints, may be NULL): residuals whose new state is IN, OOB, OUTLIER. */
int eds_win_linearize(eds_win* win, int F, const float* precalc, const float* frame_energy_th, double* energy, int32_t* counts);
/* applyRes(copy_jacobians) for every residual */
int eds_win_apply(eds_win* win, int copy_jacobians);
/* the per-point sums over the active residuals and the Schur complement's per-point prologue.  priorF[n], deltaF[n] and
 * lf[n][6] = {Hdd_accLF, bd_accLF, Hcd_accLF[4]} are inputs, finite (NULL: 0).  nres (may be NULL): the active residuals added. */
int eds_win_point_hessians(eds_win* win, const float* priorF, const float* deltaF, const float* lf, int shift_prior_to_zero, int32_t* nres);

/* eds_win_point_hessians, then every accumulator of the two addPoint()s on the device and both stitches: acc[h + F t] with its three
 * AccumulatorApprox updates, accHcc, accbc, accD[h + F t1 + F^2 t2], accE, accEB, each entry the fp64 sum of the reference's fp32 terms
 * in the order csrc/eds_window.hpp names (512 lanes striding the point index within a host frame, a fold inside every 64, the eight
 * totals left to right, hosts left to right; a point without a contribution adds +0.0); then stitchDouble with usePrior = false and
 * the Schur stitch, in fp64 in the header's order, on the device as well; the raw accumulators come back only when acc_out is given.  adHost / adTarget:
 * [h + F t][8][8] row-major doubles, finite.  H_A, H_sc: (4 + 8 F)^2 row-major; b_A, b_sc: 4 + 8 F; acc_out: the raw accumulators,
 * eds_win_acc_size(F) doubles in the header's layout (any output may be NULL).  The priors of usePrior are a diagonal add and stay
 * with the caller.  The points must be in nondecreasing host order and a point may have one residual per target. */
int eds_win_accumulate(eds_win* win, int F, const double* adHost, const double* adTarget, const float* priorF, const float* deltaF, const float* lf,
                       int shift_prior_to_zero, double* H_A, double* b_A, double* H_sc, double* b_sc, double* acc_out, int32_t* nres);
int eds_win_acc_size(int F);

int eds_win_get_residuals(eds_win* win, const eds_win_residual_out* out);
int eds_win_get_points(eds_win* win, const eds_win_point_out* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_WINDOW_H_ */
