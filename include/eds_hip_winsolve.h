/* eds_hip_winsolve.h — the rest of one Gauss-Newton iteration of DSO's window optimiser on the device, over the eds_win of
 * eds_hip_window.h: EFResidual::fixLinearizationF (reference src/bundles/EnergyFunctionalStructs.cpp:87-113), modes 1 and 2 of
 * AccumulatedTopHessianSSE::addPoint (src/bundles/AccumulatedTopHessian.cpp:40-159), EnergyFunctional::solveSystemF whole
 * (src/bundles/EnergyFunctional.cpp:775-913: the three accumulations and stitches, the priors, bM_top, both assembly branches, the scaled
 * LDLT, the orthogonalisation of x, resubstituteF_MT with the point step), setIdepth for every point, calcLEnergyF_MT, calcMEnergyF and the
 * arithmetic of marginalizePointsF (:615-669).  After eds_win_linearize / eds_win_apply one eds_wsv_solve leaves every point's step on
 * the device and returns 4 + 8 F doubles; eds_wsv_step_idepths moves the inverse depths where the next eds_win_linearize reads them.
 * The symbols are exported by libeds_hip.so; no entry point of the other headers changes.
 *
 * NOT here: marginalizeFrame, dropPointsF / removePoint and makeIDX (the caller rebuilds the tables), forming the nullspace projector
 * (the caller passes NNpiTS), the SVD branch, the momentum modes, SOLVER_ORTHOGONALIZE_POINTMARG / _FULL.
 *
 * Conventions are those of eds_hip_window.h: plain pointers, caller-owned host buffers, EDS_OK or a negative eds_status,
 * eds_last_error() for the text.  Every call returns when its results are on the device or the host.
 *  - EDS_ERR_INVALID: a NULL handle or required argument, F out of range, a value that is not finite, a mode bit that is refused.
 *  - EDS_ERR_STATE: any call before eds_wsv_set_state, or after eds_win_set_points / eds_win_set_residuals (they invalidate the state
 *    and clear every linearized flag); eds_wsv_step_idepths before a backup and a solve; eds_wsv_marginalize_points with a flagged
 *    point that has an active residual that is not linearized (the reference asserts).
 *  - EDS_ERR_NOT_USABLE: eds_wsv_solve ended with an x that is not finite; no step is written.
 *  Nothing is queued and nothing changes on EDS_ERR_INVALID or EDS_ERR_STATE.
 * No kernel uses a floating-point atomic and every sum has one fixed order (csrc/eds_winsolve.hpp states each): runs repeat exactly, and
 * the host restatement edswsv:: gives the same bits.
 *
 * The solve is a stated LDLT, not Eigen's code: fp64, the lower triangle of S H S with S = diag(1 / sqrt(H_ii + 10)), symmetric
 * pivoting on the largest |diagonal| of the trailing block (the lowest index on a tie), every dot product summed from 0 in index order
 * by one thread, a pivot that is exactly 0 gives that component 0.  One workgroup, the matrix in LDS.
 */
#ifndef EDS_HIP_WINSOLVE_H_
#define EDS_HIP_WINSOLVE_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_WINSOLVE_ABI_VERSION 1
int eds_wsv_abi_version(void);

/* setting_solverMode (reference src/utils/settings.h:35-46) */
#define EDS_WSV_SOLVER_SVD 1                      /* refused */
#define EDS_WSV_SOLVER_ORTHOGONALIZE_SYSTEM 2
#define EDS_WSV_SOLVER_ORTHOGONALIZE_POINTMARG 4  /* refused */
#define EDS_WSV_SOLVER_ORTHOGONALIZE_FULL 8       /* refused */
#define EDS_WSV_SOLVER_SVD_CUT7 16                /* refused */
#define EDS_WSV_SOLVER_REMOVE_POSEPRIOR 32        /* acts where the priors are formed: the caller's prior / priorF arrays */
#define EDS_WSV_SOLVER_USE_GN 64
#define EDS_WSV_SOLVER_FIX_LAMBDA 128
#define EDS_WSV_SOLVER_ORTHOGONALIZE_X 256
#define EDS_WSV_SOLVER_MOMENTUM 512               /* refused */
#define EDS_WSV_SOLVER_STEPMOMENTUM 1024          /* refused */
#define EDS_WSV_SOLVER_ORTHOGONALIZE_X_LATER 2048

typedef struct eds_wsv_stats {
    int32_t res_in_a, res_in_l;                   /* resInA, resInL: the residuals modes 0 and 1 added */
    int32_t orthogonalized_x, orthogonalized_system;
    double lambda;                                /* the lambda used (USE_GN: 0, FIX_LAMBDA: 1e-5) */
} eds_wsv_stats;

/* what eds_wsv_get reads back, any pointer may be NULL; m residuals, n points, F frames, N = 4 + 8 F */
typedef struct eds_wsv_out {
    float* adHTdeltaF;                            /* [h + F t][8] */
    int32_t* is_linearized;                       /* m */
    float* res_toZeroF;                           /* m x 8 */
    float* resApprox;                             /* m x 8: what the last mode 1 / 2 pass wrote (linearized active residuals) */
    float* lf;                                    /* n x 6: Hdd_accLF, bd_accLF, Hcd_accLF[4] */
    double* HFinal;                               /* N x N, HFinal_top of the last solve */
    double* bFinal;                               /* N */
    float* xAd;                                   /* [F h + t][8] */
    double* frame_step;                           /* N: -x of the last solve (HCalib->step, then every frame's step.head<8>()) */
    float* step;                                  /* n */
    float* idepth_scaled;                         /* n */
    float* priorF;                                /* n */
} eds_wsv_out;

/* setAdjointsF's float casts and setDeltaF (EnergyFunctional.cpp:90 ff., 171-194).  adHost, adTarget: [h + F t][8][8] row-major doubles as
 * eds_win_accumulate takes them; delta, prior, delta_prior: [F][8]; cPrior, cDelta: [4]; priorF, deltaF: per point (NULL: 0).  Everything
 * finite.  adHTdeltaF[h + F t][j] = sum_k (float)delta_h[k] adHostF(k, j) from 0 with k = 0 ... 7, the same for the target, the two
 * added.  Clears every linearized flag.  priorF / deltaF stay on the device in the window's own arrays: eds_win_point_hessians and
 * eds_win_accumulate called with arrays of their own REPLACE them (NULL there still means 0, not these), and called with an lf of
 * their own they replace the L sums as well: lf = NULL then means 0 again until the next eds_wsv_solve or marginalisation. */
int eds_wsv_set_state(eds_win* win, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior,
                      const double* delta_prior, const double* cPrior, const double* cDelta, const float* priorF, const float* deltaF);
/* fixLinearizationF for the residuals with select[r] != 0 (m entries): res_toZeroF from the functional's J, isLinearized = true */
int eds_wsv_fix_linearization(eds_win* win, const int32_t* select);
/* solveSystemF.  HM: N x N row-major, bM: N (finite); projector: N x N (NNpiTS) or NULL; x: N doubles out; lastHS (N x N), lastbS (N),
 * stats: may be NULL.  have_first_frame: a frame with frameID 0 is in the window (read with SOLVER_ORTHOGONALIZE_SYSTEM). */
int eds_wsv_solve(eds_win* win, int iteration, double lambda, int mode, int have_first_frame, const double* HM, const double* bM,
                  const double* projector, double* x, double* lastHS, double* lastbS, eds_wsv_stats* stats);
/* idepth_backup = idepth; then setIdepth(idepth_backup + fac * step) for every point (HessianBlocks.h:445-448) */
int eds_wsv_backup_idepths(eds_win* win);
int eds_wsv_step_idepths(eds_win* win, float fac);
int eds_wsv_get_steps(eds_win* win, float* step);
/* calcLEnergyF_MT and calcMEnergyF */
int eds_wsv_l_energy(eds_win* win, double* energy);
int eds_wsv_m_energy(eds_win* win, const double* HM, const double* bM, double* energy);
/* the arithmetic of marginalizePointsF for the points with marg[p] != 0 (n entries): priorF *= prior_fac, addPoint<2>, the Schur
 * addPoint(p, false), both stitches without priors, HM += weight_fac (M - Msc), bM += weight_fac (Mb - Mbsc) in place.
 * res_in_m (may be NULL): the residuals added. */
int eds_wsv_marginalize_points(eds_win* win, const int32_t* marg, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m);
int eds_wsv_get(eds_win* win, const eds_wsv_out* out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_WINSOLVE_H_ */
