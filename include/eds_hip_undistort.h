/* eds_hip_undistort.h — from the camera's raw uint8 / uint16 frame to the rectified, photometrically corrected fp32 plane every
 * DSO-side handle starts from, on the device.  This is dso::Undistort with its PhotometricUndistorter (reference
 * src/utils/Undistort.cpp): readFromFile from the point where the numbers are known (:782-945) with makeOptimalK_crop (:580-700) and
 * the five distortCoordinates (:961-1225), PhotometricUndistorter's constructor after the file reads (:79-170), and per frame
 * Undistort::undistort<T> (:378-474) with processFrame<T> (:206-244).  The symbols are exported by libeds_hip.so; the object is its
 * own opaque eds_und.
 *
 * Conventions are those of eds_hip_select.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, a model or output mode that does not exist, output mode "full" (the
 *    reference asserts there), sizes outside 8 .. 8192, a parameter that is not finite, mode "none" with w != w_org or h != h_org,
 *    slots outside 1 .. 16, a slot range outside the handle's, a G table that is shorter than 256, longer than 65 536 or not strictly
 *    increasing, a caller map with a pair that is neither (-1, -1) nor inside the raw image, strides that let rows or frames overlap,
 *    uint16 frames with the photometric calibration on and a G table of fewer than 65 536 entries (the reference would index past its
 *    table), and every device pointer eds_dev_check_range (include/eds_hip_device.h) refuses over exactly the extent that will be
 *    read: a wrong pointer or a wrong map is an error code and never a fault.
 *  - EDS_ERR_NOT_USABLE: the crop loop of makeOptimalK_crop passes 500 iterations (the reference calls exit(1) there).
 *  Nothing is queued and nothing changes on either of these: the planes, the map and the tables stay as they were.
 * A process that never calls eds_und_* allocates and launches nothing of this.
 *
 * Set-up runs on the HOST, inside the library, once per camera.  The geometry has tanf, atanf, atan2f and sqrtf in it, and a device
 * math library does not give the C library's bits for those; so the map is built by the host code of csrc/eds_undistort.hpp with the C
 * library's functions and uploaded, and no transcendental runs on the device.  Per frame the device then does table reads, fp32
 * products and sums only, in the reference's order and without contraction into FMAs: a plane equals the reference's bit for bit.
 * The one exception is a NaN (a zero vignette entry gives 1 / 0 = inf and, through 0 * inf, NaN, as in the reference): it is a NaN on
 * both sides, its sign and payload are the hardware's.
 *
 * Types.  Where the reference writes tan, sqrt or atan on a float argument the float function is meant (tanf, sqrtf, atanf); RadTan's
 * 2.0 * r1 * mxy_u and r2 * (rho2_u + 2.0 * mx2_u) stay products of doubles; K is a matrix of doubles that float results are stored
 * into, and -minX * K(0,0) is a product of doubles.
 *
 * Quirks of the reference that are kept (:920-925):
 *  - "if(iy == hOrg-1) ix = hOrg-1.001": ix, not iy, is moved.
 *  - the map's validity test is iy < wOrg - 1, not hOrg - 1: on a portrait sensor (h_org > w_org) rows w_org - 1 .. h_org - 2 of the
 *    raw image are never sampled.
 *  - makeOptimalK_crop tests "minX == 0" to find the first valid sample, so a first valid sample AT 0 is passed over; and its
 *    iteration count is tested after the increment whether or not the pass found anything out of bounds.
 *  - processFrame chooses its branch per frame: valid && exposure > 0 && photometric_calibration != 0 is G[raw] (times vignetteMapInv
 *    in mode 2), everything else is factor * raw.  A NaN exposure is not <= 0 and takes the photometric branch.
 * Defined rules where the reference is undefined:
 *  (1) with h_org < w_org a map pixel with h_org - 1 <= iy < w_org - 1 passes the reference's test, which then reads past the image;
 *      here such a pixel becomes (-1, -1).
 *  (2) the remap tests !(xx >= 0) where the reference tests xx < 0; the two differ for a NaN only, which no map holds.
 *  (3) eds_und_set_map on a handle of output mode "none" ends its passthrough: the caller's map is used.
 *  (4) photometric_calibration 0 overwrites G with 255.0f * i / (g_depth - 1) as the constructor does (:104-107); the table given is
 *      kept, so leaving mode 0 restores it.  Nothing per frame reads G in mode 0.
 *
 * Out of scope: applyBlurNoise and the benchmark_varNoise branch (they draw from rand() per frame and are off by default), the
 * benchmarkSetting_* overrides, unMapFloatImage, and every file and PNG read — the four lines of camera.txt are parsed by the Python
 * mirror (undistort.parse_camera_text), G and the vignette arrive as arrays.
 */
#ifndef EDS_HIP_UNDISTORT_H_
#define EDS_HIP_UNDISTORT_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_UNDISTORT_ABI_VERSION 1
int eds_und_abi_version(void);

typedef struct eds_und eds_und;

/* model = ... */
#define EDS_UND_MODEL_FOV 0
#define EDS_UND_MODEL_RADTAN 1
#define EDS_UND_MODEL_EQUIDISTANT 2
#define EDS_UND_MODEL_KB 3
#define EDS_UND_MODEL_PINHOLE 4
/* out_mode = ...: line 3 of camera.txt.  FULL exists so that a parsed file can say it; eds_und_create refuses it. */
#define EDS_UND_OUT_CROP 0
#define EDS_UND_OUT_NONE 1
#define EDS_UND_OUT_GIVEN 2
#define EDS_UND_OUT_FULL 3
/* raw_type and vignette_type = ... */
#define EDS_UND_U8 0
#define EDS_UND_U16 1
/* form = ... of eds_und_set_form */
#define EDS_UND_FORM_FUSED 0
#define EDS_UND_FORM_TWO_PASS 1
#define EDS_UND_FORM_AUTO 2
#define EDS_UND_MAX_SLOTS 16

/* what readFromFile knows after its four lines */
typedef struct eds_und_geometry {
    int32_t model;
    double pars[8];         /* parsOrg: fx fy cx cy and 1 (FOV, PINHOLE) or 4 further numbers; the unused ones are 0.  pars[2] < 1 and
                               pars[3] < 1 is the relative format and is rescaled, with the - 0.5 */
    int32_t w_org, h_org;   /* the raw image */
    int32_t out_mode;
    float out_pars[5];      /* GIVEN: fx fy cx cy relative to w and h (and a fifth number nothing reads) */
    int32_t w, h;           /* the output plane */
} eds_und_geometry;

/* setting_photometricCalibration 2 and setting_useExposure true (reference src/utils/settings.cpp:117-118) */
typedef struct eds_und_settings {
    int32_t photometric_calibration;    /* 0: factor * raw; 1: G; 2: G and the vignette */
    int32_t use_exposure;               /* 0: exposures_out is 1 */
} eds_und_settings;
void eds_und_settings_default(eds_und_settings* s);

/* K, the map and `slots` output planes of w x h floats.  Host work: two lines of 100 000 samples, the crop loop, w * h map pixels. */
int eds_und_create(int device, const eds_und_geometry* geometry, int slots, eds_und** und);
void eds_und_destroy(eds_und* und);

/* the rectified camera matrix, row-major */
int eds_und_get_K(const eds_und* und, double K[9]);
/* remapX and remapY, w * h floats each (either may be NULL): a pair is (-1, -1) or a position inside the raw image */
int eds_und_get_map(const eds_und* und, float* mapx, float* mapy);
int eds_und_is_passthrough(const eds_und* und, int* passthrough);
/* Replaces the map by the caller's (w * h floats each, host memory), e.g. the tables of cv::initUndistortRectifyMap.  Every pair is
 * (-1, -1), or finite with 0 < x < w_org - 1 and 0 < y < h_org - 1; anything else is EDS_ERR_INVALID and changes nothing. */
int eds_und_set_map(eds_und* und, const float* mapx, const float* mapy);

/* PhotometricUndistorter's constructor after its file reads.  G: g_depth floats, 256 .. 65 536 of them, strictly increasing; rescaled
 * to 0 .. 255 in double.  vignette: w_org x h_org values of vignette_type, dense; divided by their maximum in fp32, then 1.0f / v.
 * Without this call the handle is the reference's !valid. */
int eds_und_set_photometric(eds_und* und, const float* G, int g_depth, const void* vignette, int vignette_type);
int eds_und_set_settings(eds_und* und, const eds_und_settings* s);
int eds_und_get_settings(const eds_und* und, eds_und_settings* s);
/* the two device forms of the per-frame path give the same bits: FUSED (one kernel: the photometric step inside the four taps) and
 * TWO_PASS (the photometric plane, then the remap; it allocates count x w_org x h_org floats on its first use).  Neither is the faster
 * one everywhere, so the default is AUTO: FUSED for a call of fewer than 4 Mi raw pixels (count x w_org x h_org),
 * TWO_PASS from there on.  The other two values pin a form, for tests and measurements. */
int eds_und_set_form(eds_und* und, int form);
int eds_und_get_form(const eds_und* und, int* form);

/* undistort<T> for `count` frames into slots first_slot .. first_slot + count - 1; returns when the planes are on the device.
 * raw: uint8 or uint16 (raw_type) frames of w_org x h_org, rows row_stride ELEMENTS apart (0 = dense; otherwise >= w_org), frames
 * frame_stride elements apart (0 = dense; otherwise >= (h_org - 1) * row_stride + w_org).  on_device = 0: host memory; 1: device
 * memory, range-checked.  exposures: count floats (host); factor: the plain branch's scale; exposures_out (count floats, host, may be
 * NULL): the exposure, or 1 when use_exposure is off. */
int eds_und_process(eds_und* und, int first_slot, int count, const void* raw, int raw_type, int64_t row_stride, int64_t frame_stride,
                    int on_device, const float* exposures, float factor, float* exposures_out);

/* The device plane of a slot, dense (row_stride = w), for eds_ct_set_ref / set_new, eds_imm_set_*_images, eds_win_set_frames,
 * eds_sel_set_image, eds_ini_set_first / track_frame with on_device = 1.  It stays valid until eds_und_destroy and holds what the last
 * eds_und_process wrote there (zeros before the first). */
int eds_und_image(const eds_und* und, int slot, const float** d_image, int64_t* row_stride);
/* ... and read back: w * h floats */
int eds_und_get_image(eds_und* und, int slot, float* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_UNDISTORT_H_ */
