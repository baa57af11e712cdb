/* eds_hip_select.h — DSO's pixel selector on the device: which pixels of a new keyframe become immature points.  This is
 * dso::PixelSelector::makeMaps whole (reference src/mapping/PixelSelector.cpp:136-227) with makeHists (:72-135), select (:231-374) and
 * computeHistQuantil (:60-69), over levels 0, 1 and 2 of FrameHessian::makeImages (src/tracking/HessianBlocks.cpp:139-202) INCLUDING
 * absSquaredGrad, which only the selector reads.  The symbols are exported by libeds_hip.so; the object is its own opaque eds_sel.
 *
 * Conventions are those of eds_hip_immature.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.  Every call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, sizes or strides out of range, a parameter eds_sel_set_params refuses, a
 *    density or th_factor that is not positive and finite, a B table that is not finite, and every device pointer
 *    eds_dev_check_range (include/eds_hip_device.h) refuses over the extent that will be read: a wrong pointer is an error code and
 *    never a fault.
 *  - EDS_ERR_STATE: eds_sel_make_maps without a table or without an image, the getters before what they read exists.
 *  Nothing is queued and nothing changes on either of these.
 * A process that never calls eds_sel_* allocates and launches nothing of this.  No kernel uses a floating-point atomic, counts are
 * integers, and every arg-max has a total order: a run equals its repetition bit for bit.
 *
 * The random table.  The reference's selector calls rand() only in its constructor: srand(3141592), then W * H bytes rand() & 0xFF.
 * Everything after that is deterministic in the table, so the table is an INPUT here (eds_sel_set_random_pattern).
 * eds_sel_fill_reference_pattern does what the constructor does — it RESEEDS the C library's generator — and the library never
 * calls it on its own.
 *
 * Images.  Input is fp32 intensities on DSO's 0 .. 255 scale.  Level l is (W >> l) x (H >> l) — an odd width is halved as wG[] is —
 * with colour, dx, dy as eds_hip_coarse.h and eds_hip_immature.h document them (the flat-index rule, rows 0 and h - 1 are 0; the very
 * same restatement is used) and absSquaredGrad = dx * dx + dy * dy, times gw * gw with gw = B[c + 1] - B[c], c = (int)(colour + 0.5f)
 * clamped to 5 .. 250, when a B table (CalibHessian::B, setting_gammaWeightsPixelSelect == 1) is given.  absSquaredGrad of rows 0 and
 * h - 1, which the reference leaves uninitialised and never reads, is 0.
 *
 * Arithmetic and quirks.  fp32 in the order the reference writes it, no contraction into FMAs; every quirk of the reference is kept
 * and every place where it is undefined has a defined rule.  Both lists are in csrc/eds_pixsel.hpp, which the kernels and the host
 * restatement share; the defined rules in short: (1) the thsSmoothed index with W or H no multiple of 32 is the reference's flat
 * index while that is below (W / 32) (H / 32) and the clamped block otherwise; (2) (int)sqrtf(v) is 48 when the root is NaN or not
 * below 49; (3) no selected pixel gives quotia = +inf and the float rules decide; no integer is formed from a non-finite float;
 * (4) any potential 1 .. 2^30 is accepted, a 4 pot block larger than the image is one block; (5) histogram bins 50 .. 90 are 0.
 *
 * The loop that walks the map and constructs the points, FullSystem::makeNewTraces, is not in the reference tree; see
 * eds_imm_create_points_selected in eds_hip_immature.h.  CoarseInitializer's use of makePixelStatus for levels above 0 stays out.
 */
#ifndef EDS_HIP_SELECT_H_
#define EDS_HIP_SELECT_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_SELECT_ABI_VERSION 1
int eds_sel_abi_version(void);

typedef struct eds_sel eds_sel;

/* the setting_* values the selector reads (reference src/utils/settings.cpp:145-148) */
typedef struct eds_sel_params {
    float min_grad_hist_cut;                  /* setting_minGradHistCut 0.5; 0 .. 1 */
    float min_grad_hist_add;                  /* setting_minGradHistAdd 7 */
    float grad_downweight_per_level;          /* setting_gradDownweightPerLevel 0.75 */
    int32_t select_direction_distribution;    /* setting_selectDirectionDistribution 1 (0: the gradient magnitude decides) */
} eds_sel_params;
void eds_sel_params_default(eds_sel_params* p);

/* one select pass of eds_sel_make_maps: the potential it ran at and the selections at levels 0, 1, 2 */
typedef struct eds_sel_pass {
    int32_t potential, n2, n3, n4;
} eds_sel_pass;

/* which = ... of eds_sel_get_thresholds */
#define EDS_SEL_THS 0
#define EDS_SEL_THS_SMOOTHED 1
#define EDS_SEL_MAX_POTENTIAL (1 << 30)

/* H, W 32 .. 8192.  The parameters start as eds_sel_params_default, currentPotential as 3. */
int eds_sel_create(int device, int H, int W, eds_sel** sel);
void eds_sel_destroy(eds_sel* sel);
/* every float finite, min_grad_hist_cut 0 .. 1.  New parameters make the next eds_sel_make_maps histogram again. */
int eds_sel_set_params(eds_sel* sel, const eds_sel_params* p);
int eds_sel_get_params(const eds_sel* sel, eds_sel_params* p);

/* randomPattern: n = W * H bytes */
int eds_sel_set_random_pattern(eds_sel* sel, const uint8_t* table, size_t n);
/* srand(3141592), then out[i] = rand() & 0xFF: RESEEDS the C library's generator.  Never called by the library itself. */
int eds_sel_fill_reference_pattern(uint8_t* out, size_t n);

/* currentPotential, 1 .. EDS_SEL_MAX_POTENTIAL */
int eds_sel_set_potential(eds_sel* sel, int potential);
int eds_sel_get_potential(const eds_sel* sel, int* potential);

/* Levels 0 .. 2 of makeImages.  Rows row_stride elements apart (0 = dense; otherwise >= W).  on_device = 0: host memory; 1: device
 * memory, range-checked.  B: NULL for HCalib == 0, otherwise the 256 finite floats of CalibHessian::B (host memory).  A new image makes
 * the next eds_sel_make_maps histogram again and leaves the map and the selection as they are until then. */
int eds_sel_set_image(eds_sel* sel, const float* image, int64_t row_stride, int on_device, const float* B);

/* makeMaps: makeHists unless the image and the parameters are those of the last call, select at currentPotential, the quotia /
 * idealPotential rule, up to recursions_left further select passes, the random sub-selection, the update of currentPotential.
 * density > 0 and finite (numWant), th_factor > 0 and finite, recursions_left >= 0.
 * num_have_sub: the return value of makeMaps, the number of non-zero map pixels.  passes (max_passes entries, may be NULL): every select
 * pass in order, the last one's n2, n3, n4 being those makeMaps decided on; n_passes (may be NULL): their number, which is at most
 * recursions_left + 1 — more than max_passes are counted and not stored.  pass_maps (max_passes x H x W bytes, may be NULL, for tests):
 * the map after every stored select pass, before the sub-selection. */
int eds_sel_make_maps(eds_sel* sel, float density, int recursions_left, float th_factor, int* num_have_sub, eds_sel_pass* passes,
                      int max_passes, int* n_passes, uint8_t* pass_maps);

/* the map, H * W bytes: 0, or 1, 2, 4 for a pixel selected at level 0, 1, 2 */
int eds_sel_get_map(eds_sel* sel, uint8_t* out);
/* the map's non-zero pixels in row-major order: n, and (each may be NULL) uv n x {u, v}, type n floats (the map value) */
int eds_sel_get_selection(eds_sel* sel, int* n, int32_t* uv, float* type);
/* level 0 .. 2 as (H >> lvl) x (W >> lvl) x {colour, dx, dy, absSquaredGrad}, for tests and debugging */
int eds_sel_get_level(eds_sel* sel, int lvl, float* out);
/* ths or thsSmoothed of the last makeHists: (H / 32) x (W / 32) floats */
int eds_sel_get_thresholds(eds_sel* sel, int which, float* out);
/* of the last select pass: the pot cells whose selection depended on the direction drawn, and what n2 would have been from the
 * other cells alone (for tests and measurements) */
int eds_sel_get_scan_info(eds_sel* sel, int* ambiguous_cells, int* n2_certain);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_SELECT_H_ */
