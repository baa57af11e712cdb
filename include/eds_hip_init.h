/* eds_hip_init.h — DSO's two-frame initialiser on the device: dso::CoarseInitializer (reference src/init/CoarseInitializer.cpp, lines
 * quoted as :n).  It gives a run its first pose and its first inverse depths: setFirst keeps the first frame's pyramid and one point set
 * per level, trackFrame aligns every later frame to it over SE(3), the affine pair and every point's inverse depth, coarse to fine, until
 * the translation is large enough to "snap".  The symbols are exported by libeds_hip.so; the object is its own opaque eds_ini with
 * pyramids of its own, and no entry point of the other headers changes.
 *
 * Conventions are those of eds_hip_coarse.h: plain pointers and sizes, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.  Every call returns when its results are on the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, a size, level, stride or index out of range, a parameter set
 *    eds_ini_set_params refuses, an exposure or calibration that is not finite, more selected pixels than max_points_per_level, and
 *    every device pointer eds_dev_check_range (include/eds_hip_device.h) refuses over the extent that will be read: a host pointer
 *    passed with on_device = 1 is an error code and never a fault.
 *  - EDS_ERR_STATE: eds_ini_set_first before eds_ini_set_calib; eds_ini_set_neighbours before the points of the level (and of the level
 *    above) exist; eds_ini_track_frame before the first frame, every level's points and every level's tables are set; a getter before
 *    what it reads exists.
 *  Nothing is queued and nothing changes on either of these.  Every check is made before the device is touched.
 *
 * What is restated.
 *  1. makeK (:853-882) is edsct::make_k of eds_hip_coarse.h; where calcResAndGS uses the fp64 members (Ki, and cx, cy of a level) the
 *     fp64 value is formed again, and Ki is the closed form of the inverse of an upper-triangular K, not Eigen's 3 x 3 inverse.
 *  2. makeImages of both frames is eds_hip_coarse.h's item 2, by the same code.
 *  3. setFirst's point set-up (:718-749) per level from a STATUS MAP the caller passes (a float per pixel of the level; non-zero:
 *     selected, and the value is my_type): the rectangle 3 <= x < w - 4, 3 <= y < h - 4 in row-major order by a stable compaction, u =
 *     (float)(x + 0.1), idepth = iR = 1, outlierTH = 8 outlier_th.  Level 0 may come straight from an eds_sel's map in device memory.
 *     makePixelStatus / gridMaxSelection for the upper levels are eds_hip_inisetup.h's (eds_ini_make_pixel_status,
 *     eds_ini_set_points_status); a caller's own maps remain inputs here.
 *  4. makeNN's tables (:884-958) are inputs here (eds_ini_set_neighbours); eds_hip_inisetup.h makes them on the device from the
 *     level's points (eds_ini_make_neighbours).  neighboursDist and parentDist, which the reference writes and
 *     never reads, have no counterpart.  eds_ini_make_nn fills the tables on the host AS THE REFERENCE'S NANOFLANN DOES, ties
 *     included: with every point at an integer pixel + 0.1 equal fp32 distances are the normal case, and nanoflann decides them by
 *     the order its tree is visited in.  Restated from src/utils/nanoflann.h (csrc/eds_nntree.hpp): the build (:985-991, :1024-1046
 *     the root box, :1056-1104 divideTree with leaf size 5, :1118-1157 middleSplit_, :1169-1196 planeSplit), the walk (:1198-1215,
 *     :1222-1269 searchLevel: near child by diff1 + diff2 < 0, the fp32 running mindistsq with its <= prune, a leaf's dist <
 *     worst_dist against the worst distance on entry) and KNNResultSet::addPoint without NANOFLANN_FIRST_MATCH (:124-145); the
 *     distance is FLANNPointcloud::kdtree_distance, d0 d0 + d1 d1 in fp32 without contraction.  Coordinates must be finite and a
 *     parent table needs n_up >= 1 (EDS_ERR_INVALID otherwise); a parent search in which every squared distance overflows answers 0.
 *     tests/test_nn_pin.py holds this to the reference's own nanoflann (tests/golden/nn/).
 *  5. trackFrame (:75-262), whole, in ONE kernel launch and one wait: the new frame's pyramid, the un-snapped reset, the exposure guess
 *     (its logf is taken on the host), per level propagateDown, resetPoints, calcResAndGS, applyStep and the damped loop with doStep,
 *     calcEC, the accept test, the float equality that sets `snapped`, optReg, the lambda schedule and the three exits; propagateUp;
 *     frameID / snappedAt and the return value.  calcResAndGS keeps its quirks: EAlpha stays 0 (the second loop adds into E after E is
 *     finished), so alphaEnergy = alphaW |t|^2 npts, and E.num counts both loops.  Nothing per point crosses the bus.
 *  6. The loops that depend on their own order — optReg, resetPoints at the top level, propagateUp's += — give the serial loops' values:
 *     the first two run by a dependency schedule eds_ini_set_neighbours derives (csrc/eds_init.hpp), the third gathers per parent over
 *     its children in ascending order.
 *
 * Arithmetic.  fp32 per tap and per point in the reference's order, no contraction into FMAs.  Every sum over points (the 45 products
 * of acc9, E, the 45 weighted products of acc9SC, the two of calcEC) is taken in fp64 in the lane-strided order of csrc/eds_coarse.hpp
 * and cast to float where the reference holds one; the reference adds them in fp32 in serial order.  The 8 x 8 (fix_affine: 6 x 6)
 * solve is edsct's unpivoted fp64 L D L^T of the fp32 system, narrowed to float (Eigen's pivoted fp32 ldlt() is not restated); the dot
 * product of doStep is summed left to right; SE3::exp is edsct::se3_exp_mul; refToNew.log().head<3>() takes Eigen's quaternion of R,
 * Sophus's logAndTheta with the header's own plain-arithmetic atan (within 2 ulps of libm) and V^-1 t.  The host restatement
 * (edsini::SerialEv) walks the same order: it and the device agree bit for bit on everything this header returns.
 */
#ifndef EDS_HIP_INIT_H_
#define EDS_HIP_INIT_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"
#include "eds_hip_select.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_INIT_ABI_VERSION 1
int eds_ini_abi_version(void);

typedef struct eds_ini eds_ini;

#define EDS_INI_MAX_LEVELS 5
#define EDS_INI_MAX_DECISIONS 512
#define EDS_INI_MAX_ITERATIONS 100
#define EDS_INI_MAX_POINTS 65536
#define EDS_INI_NEIGHBOURS 10

typedef struct eds_ini_params {
    float huber_th;                       /* setting_huberTH 9 */
    float outlier_th;                     /* setting_outlierTH 12 * 12 */
    float alpha_k;                        /* 2.5 * 2.5 (:83) */
    float alpha_w;                        /* 150 * 150 (:84) */
    float reg_weight;                     /* 0.8 (:85) */
    float coupling_weight;                /* 1 (:86) */
    int32_t fix_affine;                   /* fixAffine, 1 */
    int32_t max_iterations[EDS_INI_MAX_LEVELS];   /* {5, 5, 10, 30, 50} (:79); each 0 .. EDS_INI_MAX_ITERATIONS */
    float scale_xi_rot;                   /* wM (:58-61): SCALE_XI_ROT 1 */
    float scale_xi_trans;                 /* SCALE_XI_TRANS 1 */
    float scale_a;                        /* SCALE_A 10 */
    float scale_b;                        /* SCALE_B 1000 */
} eds_ini_params;
void eds_ini_params_default(eds_ini_params* p);

/* one point: the reference's Pnt without its tables, 16 words */
typedef struct eds_ini_point {
    float u, v, idepth, idepth_new, iR, lastHessian, lastHessian_new, maxstep;
    float energy[2], energy_new[2];
    float my_type, outlierTH;
    int32_t isGood, isGood_new;
} eds_ini_point;

typedef struct eds_ini_result {
    double T[12];                         /* thisToNext, row-major 3 x 4 [R | t] */
    double aff[2];                        /* thisToNext_aff (a, b) */
    float latest_res[3];                  /* resOld of level 0: E, alphaEnergy, E.num */
    float rescale;                        /* rescale() (:526) */
    int32_t snapped, frame_id, snapped_at;
    int32_t ready;                        /* the bool trackFrame returns */
    int32_t n_decisions;
    int32_t launches, waits;              /* kernel launches and stream waits of this call: 1 and 1 */
    int32_t reserved;
    int32_t iterations[EDS_INI_MAX_LEVELS];
    int32_t accepts[EDS_INI_MAX_LEVELS];
    uint8_t decisions[EDS_INI_MAX_DECISIONS];     /* per iteration, in order: bit 0 accept, bits 1 .. the level */
} eds_ini_result;

/* levels 1 .. 5; H, W as eds_ct_create takes them; max_points_per_level 1 .. EDS_INI_MAX_POINTS */
int eds_ini_create(int device, int H, int W, int levels, int max_points_per_level, eds_ini** ini);
void eds_ini_destroy(eds_ini* ini);
/* every float finite; huber_th, outlier_th and the four scales positive; fix_affine 0 or 1; max_iterations 0 .. 100 */
int eds_ini_set_params(eds_ini* ini, const eds_ini_params* p);
int eds_ini_get_params(const eds_ini* ini, eds_ini_params* p);
int eds_ini_set_calib(eds_ini* ini, float fx, float fy, float cx, float cy);

/* The first frame (fp32, DSO's 0 .. 255 scale; rows row_stride elements apart, 0 = W; on_device = 1: device memory, range-checked)
 * and its ab_exposure.  thisToNext becomes the identity, snapped 0, frameID and snappedAt 0 (:766-768); thisToNext_aff stays what it is, as in the
 * reference ((0, 0) on a new handle). */
int eds_ini_set_first(eds_ini* ini, const float* image, int64_t row_stride, int on_device, float exposure);

/* thisToNext and thisToNext_aff (public members of the reference's class): the guess the next eds_ini_track_frame starts from.  T is
 * row-major 3 x 4 [R | t], finite. */
int eds_ini_set_pose(eds_ini* ini, const double* T, const double* aff);

/* One level's points from a status map of the level's size (h x w floats, rows row_stride apart, 0 = w).  n_out: the number of points.
 * The level's tables, and those of the level below (its parents), are forgotten. */
int eds_ini_set_points(eds_ini* ini, int lvl, const float* status, int64_t row_stride, int on_device, int32_t* n_out);
/* level 0 from the map the selector's last eds_sel_make_maps left in device memory (same device, same H x W), without a read-back */
int eds_ini_set_points_selected(eds_ini* ini, eds_sel* sel, int32_t* n_out);

/* makeNN's tables of one level: neighbours n x 10 (indices into the level, -1: none), parent n (indices into level lvl + 1; NULL at
 * the top level).  Every index is checked on the host. */
int eds_ini_set_neighbours(eds_ini* ini, int lvl, const int32_t* neighbours, const int32_t* parent);
/* fills such tables on the host — nanoflann's, ties included (item 4): uv n x {u, v} of the level, uv_up n_up x {u, v} of the level
 * above (NULL / 0 and parent NULL at the top level).  Fewer than 10 points: the rest of a row is -1. */
int eds_ini_make_nn(int n, const float* uv, int n_up, const float* uv_up, int32_t* neighbours, int32_t* parent);
/* the depths of a level's dependency schedule (what optReg and resetPoints cost in barriers) */
int eds_ini_get_schedule_depth(const eds_ini* ini, int lvl, int32_t* depth_out);

/* trackFrame for one new frame */
int eds_ini_track_frame(eds_ini* ini, const float* image, int64_t row_stride, int on_device, float exposure, int snapped_threshold,
                        eds_ini_result* out);

/* the device time of the last eds_ini_track_frame's kernel in milliseconds (two events around its launch) */
int eds_ini_get_kernel_ms(const eds_ini* ini, float* ms_out);

/* read-backs, for tests and for the hand-over: the points of a level (n_out may be NULL); one of its Jacobian buffers, n x 10
 * (which = 0: JbBuffer, 1: JbBuffer_new); a pyramid level, h x w x {colour, dx, dy} (which = 0: the first frame, 1: the newest) */
int eds_ini_get_points(eds_ini* ini, int lvl, eds_ini_point* out, int32_t* n_out);
int eds_ini_get_jb(eds_ini* ini, int lvl, int which, float* out);
int eds_ini_get_level(eds_ini* ini, int which, int lvl, float* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_INIT_H_ */
