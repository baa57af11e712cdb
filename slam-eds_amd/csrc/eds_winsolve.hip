// include/eds_hip_winsolve.h: the rest of one Gauss-Newton iteration of the window optimiser on the device.  The arithmetic is
// eds_winsolve.hpp, shared with the host; this file holds the kernels and the C entry points.  Built without contraction into FMAs
// (csrc/Makefile).  Everything of one call runs in the window's stream, in order; the accumulators, the stitched matrices and the
// assembled system stay on the device.
//
// k_wsv_fix and k_wsv_res_approx give a residual EIGHT lanes, as k_win_apply has: lane j forms tap j; the two Jp_delta dots are the same
// in the eight lanes.  resApprox is written once per residual, and edswin::top_term reads it for every accumulator word.
// k_wsv_solve is one workgroup: edswsv::solve_body with the matrix and the factor in LDS — a serial chain by design (68 pivot steps with
// three barriers each); it is on the device because the steps never leave it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_winsolve.h"
#include "eds_capi_internal.hpp"
#include "eds_window_internal.hpp"
#include "eds_winsolve.hpp"

using edscapi::blocks;
using edscapi::fail;
using edscapi::read_back;
using edswin::PointOut;
using edswsv::Lin;
using edswsv::MAX_N;

namespace {

constexpr int TB = 256, SOLVE_TB = 128;

__global__ void __launch_bounds__(TB) k_wsv_fix(Lin t, int m, const int32_t* __restrict__ select, float* __restrict__ rtz, int32_t* __restrict__ lin) {
    const int gid = blockIdx.x * TB + threadIdx.x, r = gid >> 3, j = gid & 7;
    if (r >= m || !select[r]) return;
    rtz[(size_t)r * 8 + j] = edswsv::fix_tap(t, r, j);
    if (j == 0) lin[r] = 1;
}

__global__ void __launch_bounds__(TB) k_wsv_res_approx(Lin t, int m, int mode, float* __restrict__ out) {
    const int gid = blockIdx.x * TB + threadIdx.x, r = gid >> 3, j = gid & 7;
    if (r >= m || !t.lin[r]) return;
    out[(size_t)r * 8 + j] = edswsv::res_approx_tap(t, mode, r, j);
}

// Hdd_accLF, bd_accLF, Hcd_accLF of modes 1 / 2, one thread per point; the count of residuals added is an integer atomic
__global__ void __launch_bounds__(TB) k_wsv_lf(Lin t, int n, int mode, const int32_t* __restrict__ sel, float* __restrict__ lf, int32_t* count) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= n || (sel && !sel[p])) return;
    float o[6];
    const int added = edswsv::lf_sums(t, mode, p, o);
#pragma unroll
    for (int k = 0; k < 6; ++k) lf[6 * p + k] = o[k];
    if (added) atomicAdd(count, added);
}

__global__ void __launch_bounds__(TB) k_wsv_assemble(edswsv::Sys s, int stage) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e < s.N * (s.N + 1)) edswsv::assemble(s, stage, e);
}

struct DevSync { __device__ void operator()() const { __syncthreads(); } };

__global__ void __launch_bounds__(SOLVE_TB) k_wsv_solve(edswsv::SolveIo io) {
    __shared__ edswsv::SolveMem mem;
    edswsv::solve_body(io, mem, (int)threadIdx.x, SOLVE_TB, DevSync());
}

// resubstituteFPt, one thread per point, xAd and cstep in LDS; nothing is written when the solve flagged its x
__global__ void __launch_bounds__(TB) k_wsv_step(Lin t, int n, const PointOut* __restrict__ pout, const float* __restrict__ lf, const float* __restrict__ JpJdF,
                                                 const float* __restrict__ xAd, const int32_t* __restrict__ flag, float* __restrict__ step) {
    __shared__ float sh[edswin::MAX_FRAMES * edswin::MAX_FRAMES * 8 + 4];
    if (flag[0]) return;
    for (int k = threadIdx.x; k < t.F * t.F * 8 + 4; k += TB) sh[k] = xAd[k];
    __syncthreads();
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    float l[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) l[k] = lf[6 * p + k];
    step[p] = edswsv::point_step(t, pout[p], l, JpJdF, sh, p);
}

__global__ void __launch_bounds__(TB) k_wsv_backup(int n, float scale, const float* __restrict__ ids, float* __restrict__ backup) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n) backup[p] = edswsv::idepth_of(ids[p], scale);
}
__global__ void __launch_bounds__(TB) k_wsv_step_idepths(int n, float scale, float fac, const float* __restrict__ backup, const float* __restrict__ step,
                                                         float* __restrict__ ids) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n) ids[p] = edswsv::stepped_idepth_scaled(backup[p], fac, step[p], scale);
}

// setDeltaF's per-point part from the device's inverse depths (EnergyFunctional.cpp:190)
__global__ void __launch_bounds__(TB) k_wsv_delta_of_idepths(int n, float scale, const float* __restrict__ ids, const float* __restrict__ idz, float* __restrict__ delta) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n) delta[p] = edswsv::delta_of_idepths(ids[p], idz[p], scale);
}

// calcLEnergyF_MT: per host frame the 512 lanes stride its points and fold as csrc/eds_window.hpp says, hosts left to right, then the priors
__global__ void __launch_bounds__(edswin::LANES) k_wsv_l_energy(Lin t, const int32_t* __restrict__ first, const double* __restrict__ vec, const float* __restrict__ cF,
                                                               double* out) {
    __shared__ double part[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0;
    for (int h = 0; h < t.F; ++h) {
        double v = 0.0;
        for (int p = first[h] + (int)threadIdx.x; p < first[h + 1]; p += edswin::LANES) v += edswsv::lenergy_point(t, p);
        v = edsdso::wave_fold(v);
        if (lane == 0) part[wave] = v;
        __syncthreads();
        if (threadIdx.x == 0) total += edsdso::add8(part);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = edswsv::lenergy_priors(t.F, vec, cF) + total;
}

__global__ void __launch_bounds__(SOLVE_TB) k_wsv_m_energy(int N, const double* __restrict__ HM, const double* __restrict__ bM, const double* __restrict__ delta,
                                                          double* out) {
    __shared__ double row[MAX_N];
    for (int i = threadIdx.x; i < N; i += SOLVE_TB) row[i] = edswsv::menergy_row(N, HM, bM, delta, i);
    __syncthreads();
    if (threadIdx.x == 0) {
        double e = 0.0;
        for (int i = 0; i < N; ++i) e += delta[i] * row[i];
        out[0] = e;
    }
}

// marginalizePointsF's guard: flagged points' active residuals that are not linearized
__global__ void __launch_bounds__(TB) k_wsv_marg_check(int m, const int32_t* __restrict__ res_point, const int32_t* __restrict__ active,
                                                       const int32_t* __restrict__ lin, const int32_t* __restrict__ sel, int32_t* count) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m && sel[res_point[r]] && active[r] && !lin[r]) atomicAdd(count, 1);
}
__global__ void __launch_bounds__(TB) k_wsv_scale_prior(int n, const int32_t* __restrict__ sel, float fac, float* __restrict__ prior) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n && sel[p]) prior[p] *= fac;
}
// HM += w (M - Msc), bM += w (Mb - Mbsc); st: H_A, b_A, H_sc, b_sc of the stitch, io: HM (N N) then bM (N)
__global__ void __launch_bounds__(TB) k_wsv_marg_add(int N, double w, const double* __restrict__ st, double* __restrict__ io) {
    const int e = blockIdx.x * TB + threadIdx.x, half = N * (N + 1);
    if (e < half) io[e] = io[e] + w * (st[e] - st[half + e]);
}

bool finite_all(const double* x, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; }
bool finite_all(const float* x, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; }

int check(const eds_win* h) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!h->wsv || !h->wsv->valid) return fail(EDS_ERR_STATE, "eds_wsv: no state set (eds_wsv_set_state; eds_win_set_points and eds_win_set_residuals invalidate it)");
    return EDS_OK;
}
Lin lin_of(const eds_win* h) {
    const eds_wsv_state* s = h->wsv;
    Lin t = {s->F, h->res_first, h->res_point, h->res_target, h->active, s->lin, h->pts, h->efJ, s->rtz, s->res_approx, s->adHTdeltaF, s->cF, h->delta, h->prior};
    return t;
}
int alloc_state(eds_win* h) {
    if (h->wsv) return EDS_OK;
    eds_wsv_state* s = new eds_wsv_state;
    const size_t mp = (size_t)h->max_points, mr = (size_t)h->max_residuals, ms = mp > mr ? mp : mr;
    const bool ok = h->own.alloc({{(void**)&s->lin, mr * sizeof(int32_t)},
                                  {(void**)&s->sel, ms * sizeof(int32_t)},
                                  {(void**)&s->rtz, mr * 8 * sizeof(float)},
                                  {(void**)&s->res_approx, mr * 8 * sizeof(float)},
                                  {(void**)&s->adF, 2 * 64 * 64 * sizeof(float)},
                                  {(void**)&s->adHTdeltaF, 64 * 8 * sizeof(float)},
                                  {(void**)&s->cF, 8 * sizeof(float)},
                                  {(void**)&s->xAd, (64 * 8 + 4) * sizeof(float)},
                                  {(void**)&s->step, mp * sizeof(float)},
                                  {(void**)&s->backup, mp * sizeof(float)},
                                  {(void**)&s->ad, 2 * 64 * 64 * sizeof(double)},
                                  {(void**)&s->vec, 4 * MAX_N * sizeof(double)},
                                  {(void**)&s->accL, (size_t)edswin::acc_size(8) * sizeof(double)},
                                  {(void**)&s->stL, (size_t)MAX_N * (MAX_N + 1) * sizeof(double)},
                                  {(void**)&s->work, (size_t)edswsv::work_words() * sizeof(double)},
                                  {(void**)&s->flag, 4 * sizeof(int32_t)},
                                  {(void**)&s->e_out, 2 * sizeof(double)}});
    if (!ok) {                                                  // nothing half-allocated stays behind: the next call allocates again
        delete s;
        return fail(EDS_ERR_HIP, "eds_wsv_set_state: the device refused an allocation");
    }
    h->wsv = s;
    return EDS_OK;
}

}  // namespace

namespace edswin_internal {

void wsv_release(eds_win* h) {
    delete h->wsv;
    h->wsv = nullptr;
}

void wsv_invalidate(eds_win* h) {
    if (!h->wsv) return;
    h->wsv->rows_live = false;
    h->wsv->valid = false; h->wsv->lf_on_device = false; h->wsv->have_backup = false; h->wsv->have_step = false; h->wsv->have_system = false;
}

// eds_wsv_set_state, and with from_device eds_wed_set_state (include/eds_hip_winedit.h): deltaF from the device's inverse depths, and,
// where a state was set since the last eds_win_set_points / eds_win_set_residuals, priorF, isLinearized and res_toZeroF kept
int wsv_set_state(eds_win* h, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior, const double* delta_prior,
                  const double* cPrior, const double* cDelta, const float* priorF, const float* deltaF, bool from_device) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (F < 2 || F > h->max_frames) return fail(EDS_ERR_INVALID, "F is 2 .. max_frames");
    if (!adHost || !adTarget || !delta || !prior || !delta_prior || !cPrior || !cDelta)
        return fail(EDS_ERR_INVALID, "adHost, adTarget, delta, prior, delta_prior, cPrior and cDelta are required");
    if (h->max_host >= F || h->max_target >= F) return fail(EDS_ERR_INVALID, "a point's host or a residual's target is not below F");
    const size_t adw = (size_t)F * F * 64, n = (size_t)h->n;
    if (!finite_all(adHost, adw) || !finite_all(adTarget, adw) || !finite_all(delta, 8 * (size_t)F) || !finite_all(prior, 8 * (size_t)F) ||
        !finite_all(delta_prior, 8 * (size_t)F) || !finite_all(cPrior, 4) || !finite_all(cDelta, 4) || (priorF && !finite_all(priorF, n)) ||
        (deltaF && !finite_all(deltaF, n)))
        return fail(EDS_ERR_INVALID, "eds_wsv_set_state: an input is not finite");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = alloc_state(h)) return rc;
    eds_wsv_state* s = h->wsv;
    const bool keep = from_device && s->rows_live;              // include/eds_hip_winedit.h: priorF, isLinearized and res_toZeroF stay
    // the float casts and setDeltaF on the host, by the code the oracle runs (a few thousand operations)
    std::vector<float> adF(2 * adw), adht((size_t)F * F * 8), cF(8);
    for (size_t i = 0; i < adw; ++i) { adF[i] = (float)adHost[i]; adF[adw + i] = (float)adTarget[i]; }
    for (int hh = 0; hh < F; ++hh)
        for (int t = 0; t < F; ++t) {
            const size_t idx = (size_t)hh + (size_t)F * t;
            edswsv::adht_delta(adF.data() + 64 * idx, adF.data() + adw + 64 * idx, delta + 8 * hh, delta + 8 * t, adht.data() + 8 * idx);
        }
    std::vector<double> ad(2 * adw), vec((size_t)4 * MAX_N, 0.0);
    std::memcpy(ad.data(), adHost, adw * sizeof(double));
    std::memcpy(ad.data() + adw, adTarget, adw * sizeof(double));
    for (int k = 0; k < 4; ++k) {
        cF[k] = (float)cDelta[k]; cF[4 + k] = (float)cPrior[k];
        vec[k] = (double)cF[k]; vec[MAX_N + k] = cPrior[k]; vec[2 * MAX_N + k] = cPrior[k] * (double)cF[k]; vec[3 * MAX_N + k] = (double)cF[k];
    }
    for (int i = 0; i < 8 * F; ++i) {
        vec[4 + i] = delta[i]; vec[MAX_N + 4 + i] = prior[i]; vec[2 * MAX_N + 4 + i] = prior[i] * delta_prior[i]; vec[3 * MAX_N + 4 + i] = delta_prior[i];
    }
    hipStream_t st = h->own.st;
    EDS_HIP_TRY(hipMemcpyAsync(s->adF, adF.data(), adF.size() * sizeof(float), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemcpyAsync(s->adHTdeltaF, adht.data(), adht.size() * sizeof(float), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemcpyAsync(s->cF, cF.data(), 8 * sizeof(float), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemcpyAsync(s->ad, ad.data(), ad.size() * sizeof(double), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemcpyAsync(s->vec, vec.data(), vec.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (n) {
        if (priorF) EDS_HIP_TRY(hipMemcpyAsync(h->prior, priorF, n * sizeof(float), hipMemcpyHostToDevice, st));
        else if (!keep) EDS_HIP_TRY(hipMemsetAsync(h->prior, 0, n * sizeof(float), st));
        if (from_device) {
            hipLaunchKernelGGL(k_wsv_delta_of_idepths, dim3(blocks(n)), dim3(TB), 0, st, h->n, h->prm.scale_idepth, h->ids, h->idz, h->delta);
            EDS_HIP_TRY(hipGetLastError());
        } else if (deltaF) {
            EDS_HIP_TRY(hipMemcpyAsync(h->delta, deltaF, n * sizeof(float), hipMemcpyHostToDevice, st));
        } else {
            EDS_HIP_TRY(hipMemsetAsync(h->delta, 0, n * sizeof(float), st));
        }
        EDS_HIP_TRY(hipMemsetAsync(h->lf, 0, 6 * n * sizeof(float), st));
        EDS_HIP_TRY(hipMemsetAsync(s->step, 0, n * sizeof(float), st));
    }
    if (h->m) {
        if (!keep) {
            EDS_HIP_TRY(hipMemsetAsync(s->lin, 0, (size_t)h->m * sizeof(int32_t), st));
            EDS_HIP_TRY(hipMemsetAsync(s->rtz, 0, (size_t)h->m * 8 * sizeof(float), st));
        }
        EDS_HIP_TRY(hipMemsetAsync(s->res_approx, 0, (size_t)h->m * 8 * sizeof(float), st));
    }
    EDS_HIP_TRY(hipStreamSynchronize(st));
    s->F = F; s->valid = true; s->rows_live = true; s->lf_on_device = false; s->have_backup = false; s->have_step = false; s->have_system = false;
    return EDS_OK;
}

}  // namespace edswin_internal

extern "C" {

int eds_wsv_abi_version(void) { return EDS_HIP_WINSOLVE_ABI_VERSION; }

int eds_wsv_set_state(eds_win* h, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior,
                      const double* delta_prior, const double* cPrior, const double* cDelta, const float* priorF, const float* deltaF) {
    return edswin_internal::wsv_set_state(h, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta, priorF, deltaF, false);
}

int eds_wsv_fix_linearization(eds_win* h, const int32_t* select) {
    if (int rc = check(h)) return rc;
    if (!select && h->m) return fail(EDS_ERR_INVALID, "select is required");
    if (!h->m) return EDS_OK;
    eds_wsv_state* s = h->wsv;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(s->sel, select, (size_t)h->m * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    edswin_internal::wsv_queue_fix(h, s->sel);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_wsv_solve(eds_win* h, int iteration, double lambda, int mode, int have_first_frame, const double* HM, const double* bM,
                  const double* projector, double* x, double* lastHS, double* lastbS, eds_wsv_stats* stats) {
    if (int rc = check(h)) return rc;
    eds_wsv_state* s = h->wsv;
    const int F = s->F, N = 4 + 8 * F;
    const size_t NN = (size_t)N * N;
    if (!edswsv::mode_valid(mode)) return fail(EDS_ERR_INVALID, "eds_wsv_solve: the SVD, momentum, POINTMARG and FULL solver modes are not built");
    if (iteration < 0 || !std::isfinite(lambda) || lambda < 0) return fail(EDS_ERR_INVALID, "iteration >= 0, lambda finite and >= 0");
    if (have_first_frame != 0 && have_first_frame != 1) return fail(EDS_ERR_INVALID, "have_first_frame is 0 or 1");
    if (!HM || !bM || !x) return fail(EDS_ERR_INVALID, "HM, bM and x are required");
    if (!finite_all(HM, NN) || !finite_all(bM, (size_t)N) || (projector && !finite_all(projector, NN)))
        return fail(EDS_ERR_INVALID, "eds_wsv_solve: HM, bM or the projector is not finite");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edswin_internal::upload_maps(h, F)) return rc;
    lambda = edswsv::mode_lambda(mode, lambda);
    const int system = (mode & edswsv::SOLVER_ORTHOGONALIZE_SYSTEM) ? 1 : 0;
    const int orth_system = system && !have_first_frame && projector ? 1 : 0;
    const int orth_x = edswsv::mode_orth_x(mode, iteration) && projector ? 1 : 0;
    hipStream_t st = h->own.st;
    edswsv::Sys sys = {N, system, orth_system, lambda, h->stitched, h->stitched + NN, h->stitched + NN + N, h->stitched + 2 * NN + N, s->stL, s->stL + NN,
                       s->vec, s->work};
    EDS_HIP_TRY(hipMemcpyAsync(sys.mat(edswsv::W_HM), HM, NN * sizeof(double), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemcpyAsync(sys.v(edswsv::V_BM), bM, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
    if (projector) EDS_HIP_TRY(hipMemcpyAsync(sys.mat(edswsv::W_P), projector, NN * sizeof(double), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemsetAsync(s->flag, 0, 4 * sizeof(int32_t), st));
    const Lin t = lin_of(h);
    // accumulateLF: resApprox once per residual, the L sums per point, the accumulators, the stitch (its priors are the assembly's)
    if (h->m) hipLaunchKernelGGL(k_wsv_res_approx, dim3(blocks((size_t)h->m * 8)), dim3(TB), 0, st, t, h->m, 1, s->res_approx);
    if (h->n) hipLaunchKernelGGL(k_wsv_lf, dim3(blocks((size_t)h->n)), dim3(TB), 0, st, t, h->n, 1, (const int32_t*)nullptr, h->lf, s->flag + 1);
    s->lf_on_device = true;
    edswin_internal::queue_acc(h, F, 1, nullptr, 1, F * F * edswin::TOP_WORDS, s->accL);
    edswin_internal::queue_stitch(h, F, s->accL, s->ad, N * (N + 1), s->stL);
    // accumulateAF and accumulateSCF (shiftPriorToZero = true)
    edswin_internal::queue_points(h, 0, nullptr, 1);
    edswin_internal::queue_acc(h, F, 0, nullptr, 1, edswin::acc_size(F), h->acc);
    edswin_internal::queue_stitch(h, F, h->acc, s->ad, edswin::stitch_words(F), h->stitched);
    const unsigned ab = blocks((size_t)N * (N + 1));
    hipLaunchKernelGGL(k_wsv_assemble, dim3(ab), dim3(TB), 0, st, sys, 0);
    if (system) {
        if (orth_system) {
            hipLaunchKernelGGL(k_wsv_assemble, dim3(ab), dim3(TB), 0, st, sys, 1);
            hipLaunchKernelGGL(k_wsv_assemble, dim3(ab), dim3(TB), 0, st, sys, 2);
        }
        hipLaunchKernelGGL(k_wsv_assemble, dim3(ab), dim3(TB), 0, st, sys, 3);
    }
    const edswsv::SolveIo io = {N, F, orth_x, sys.mat(edswsv::W_HF), sys.v(edswsv::V_BF), sys.mat(edswsv::W_P), s->adF, sys.v(edswsv::V_X), s->xAd, s->flag,
                                nullptr, nullptr};
    hipLaunchKernelGGL(k_wsv_solve, dim3(1), dim3(SOLVE_TB), 0, st, io);
    if (h->n) hipLaunchKernelGGL(k_wsv_step, dim3(blocks((size_t)h->n)), dim3(TB), 0, st, t, h->n, h->pout, h->lf, h->JpJdF, s->xAd, s->flag, s->step);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<double> back(2 * NN + 2 * (size_t)N);
    int32_t flag[4] = {0, 0, 0, 0}, res_a = 0;
    EDS_HIP_TRY(hipMemcpyAsync(back.data(), sys.v(edswsv::V_X), (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    if (lastHS) EDS_HIP_TRY(hipMemcpyAsync(back.data() + N, sys.mat(edswsv::W_LASTH), NN * sizeof(double), hipMemcpyDeviceToHost, st));
    if (lastbS) EDS_HIP_TRY(hipMemcpyAsync(back.data() + N + NN, sys.v(edswsv::V_LASTB), (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipMemcpyAsync(flag, s->flag, sizeof(flag), hipMemcpyDeviceToHost, st));
    if (h->n) EDS_HIP_TRY(hipMemcpyAsync(&res_a, h->nres, sizeof(res_a), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(x, back.data(), (size_t)N * sizeof(double));
    if (lastHS) std::memcpy(lastHS, back.data() + N, NN * sizeof(double));
    if (lastbS) std::memcpy(lastbS, back.data() + N + NN, (size_t)N * sizeof(double));
    if (stats) { stats->res_in_a = res_a; stats->res_in_l = flag[1]; stats->orthogonalized_x = orth_x; stats->orthogonalized_system = orth_system; stats->lambda = lambda; }
    s->have_system = true;
    s->last_x.assign(x, x + N);
    if (flag[0]) return fail(EDS_ERR_NOT_USABLE, "eds_wsv_solve: x is not finite; no step was written");
    s->have_step = true;
    return EDS_OK;
}

int eds_wsv_backup_idepths(eds_win* h) {
    if (int rc = check(h)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (h->n) {
        hipLaunchKernelGGL(k_wsv_backup, dim3(blocks((size_t)h->n)), dim3(TB), 0, h->own.st, h->n, h->prm.scale_idepth, h->ids, h->wsv->backup);
        EDS_HIP_TRY(hipGetLastError());
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    }
    h->wsv->have_backup = true;
    return EDS_OK;
}

int eds_wsv_step_idepths(eds_win* h, float fac) {
    if (int rc = check(h)) return rc;
    if (!std::isfinite(fac)) return fail(EDS_ERR_INVALID, "fac is not finite");
    if (!h->wsv->have_backup || !h->wsv->have_step) return fail(EDS_ERR_STATE, "eds_wsv_step_idepths needs eds_wsv_backup_idepths and a usable eds_wsv_solve first");
    if (!h->n) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    hipLaunchKernelGGL(k_wsv_step_idepths, dim3(blocks((size_t)h->n)), dim3(TB), 0, h->own.st, h->n, h->prm.scale_idepth, fac, h->wsv->backup, h->wsv->step, h->ids);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_wsv_get_steps(eds_win* h, float* step) {
    if (int rc = check(h)) return rc;
    if (!step) return fail(EDS_ERR_INVALID, "null output");
    return read_back(h->own, step, h->wsv->step, (size_t)h->n * sizeof(float));
}

int eds_wsv_l_energy(eds_win* h, double* energy) {
    if (int rc = check(h)) return rc;
    if (!energy) return fail(EDS_ERR_INVALID, "null output");
    eds_wsv_state* s = h->wsv;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edswin_internal::upload_maps(h, s->F)) return rc;
    hipLaunchKernelGGL(k_wsv_l_energy, dim3(1), dim3(edswin::LANES), 0, h->own.st, lin_of(h), h->first, s->vec, s->cF, s->e_out);
    EDS_HIP_TRY(hipGetLastError());
    return read_back(h->own, energy, s->e_out, sizeof(double));
}

int eds_wsv_m_energy(eds_win* h, const double* HM, const double* bM, double* energy) {
    if (int rc = check(h)) return rc;
    if (!HM || !bM || !energy) return fail(EDS_ERR_INVALID, "HM, bM and the output are required");
    eds_wsv_state* s = h->wsv;
    const int N = 4 + 8 * s->F;
    const size_t NN = (size_t)N * N;
    if (!finite_all(HM, NN) || !finite_all(bM, (size_t)N)) return fail(EDS_ERR_INVALID, "eds_wsv_m_energy: HM or bM is not finite");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    double* dHM = s->work + (size_t)edswsv::W_HM * MAX_N * MAX_N;
    double* dbM = s->work + (size_t)edswsv::W_MATS * MAX_N * MAX_N + (size_t)edswsv::V_BM * MAX_N;
    EDS_HIP_TRY(hipMemcpyAsync(dHM, HM, NN * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(dbM, bM, (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    hipLaunchKernelGGL(k_wsv_m_energy, dim3(1), dim3(SOLVE_TB), 0, h->own.st, N, dHM, dbM, s->vec, s->e_out + 1);
    EDS_HIP_TRY(hipGetLastError());
    return read_back(h->own, energy, s->e_out + 1, sizeof(double));
}

int eds_wsv_marginalize_points(eds_win* h, const int32_t* marg, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m) {
    if (int rc = check(h)) return rc;
    if (!HM || !bM || (!marg && h->n)) return fail(EDS_ERR_INVALID, "marg, HM and bM are required");
    return edswin_internal::wsv_marginalize_points(h, marg, prior_fac, weight_fac, HM, bM, res_in_m);
}

}  // extern "C"

namespace edswin_internal {

void wsv_queue_fix(eds_win* h, const int32_t* select) {
    if (!h->m) return;
    hipLaunchKernelGGL(k_wsv_fix, dim3(blocks((size_t)h->m * 8)), dim3(TB), 0, h->own.st, lin_of(h), h->m, select, h->wsv->rtz, h->wsv->lin);
}

int wsv_marginalize_points(eds_win* h, const int32_t* marg, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m) {
    if (int rc = check(h)) return rc;
    if (!HM || !bM) return fail(EDS_ERR_INVALID, "HM and bM are required");
    eds_wsv_state* s = h->wsv;
    const int F = s->F, N = 4 + 8 * F;
    const size_t NN = (size_t)N * N;
    if (!std::isfinite(prior_fac) || !std::isfinite(weight_fac) || !finite_all(HM, NN) || !finite_all(bM, (size_t)N))
        return fail(EDS_ERR_INVALID, "eds_wsv_marginalize_points: a factor, HM or bM is not finite");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edswin_internal::upload_maps(h, F)) return rc;
    hipStream_t st = h->own.st;
    int32_t flag[4] = {0, 0, 0, 0};
    EDS_HIP_TRY(hipMemsetAsync(s->flag, 0, 4 * sizeof(int32_t), st));
    if (h->n && marg) EDS_HIP_TRY(hipMemcpyAsync(s->sel, marg, (size_t)h->n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (h->m) {
        hipLaunchKernelGGL(k_wsv_marg_check, dim3(blocks((size_t)h->m)), dim3(TB), 0, st, h->m, h->res_point, h->active, s->lin, s->sel, s->flag + 2);
        EDS_HIP_TRY(hipGetLastError());
    }
    if (int rc = read_back(h->own, flag, s->flag, sizeof(flag))) return rc;
    if (flag[2]) return fail(EDS_ERR_STATE, "eds_wsv_marginalize_points: " + std::to_string(flag[2]) + " active residuals of the flagged points are not linearized");
    const Lin t = lin_of(h);
    double* io = s->work + (size_t)edswsv::W_T1 * MAX_N * MAX_N;                // HM then bM, N (N + 1) words over two matrix slots
    EDS_HIP_TRY(hipMemcpyAsync(io, HM, NN * sizeof(double), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemcpyAsync(io + NN, bM, (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
    if (h->n) {
        if (!s->lf_on_device) EDS_HIP_TRY(hipMemsetAsync(h->lf, 0, 6 * (size_t)h->n * sizeof(float), st));
        hipLaunchKernelGGL(k_wsv_scale_prior, dim3(blocks((size_t)h->n)), dim3(TB), 0, st, h->n, s->sel, prior_fac, h->prior);
        if (h->m) hipLaunchKernelGGL(k_wsv_res_approx, dim3(blocks((size_t)h->m * 8)), dim3(TB), 0, st, t, h->m, 2, s->res_approx);
        hipLaunchKernelGGL(k_wsv_lf, dim3(blocks((size_t)h->n)), dim3(TB), 0, st, t, h->n, 2, s->sel, h->lf, s->flag + 1);
    }
    s->lf_on_device = true;
    edswin_internal::queue_points(h, 2, s->sel, 0);
    edswin_internal::queue_acc(h, F, 2, s->sel, 1, edswin::acc_size(F), h->acc);
    edswin_internal::queue_stitch(h, F, h->acc, s->ad, edswin::stitch_words(F), h->stitched);
    hipLaunchKernelGGL(k_wsv_marg_add, dim3(blocks((size_t)N * (N + 1))), dim3(TB), 0, st, N, weight_fac, h->stitched, io);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<double> back(NN + (size_t)N);
    EDS_HIP_TRY(hipMemcpyAsync(back.data(), io, back.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipMemcpyAsync(flag, s->flag, sizeof(flag), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(HM, back.data(), NN * sizeof(double));
    std::memcpy(bM, back.data() + NN, (size_t)N * sizeof(double));
    if (res_in_m) *res_in_m = flag[1];
    return EDS_OK;
}

}  // namespace edswin_internal

extern "C" {

int eds_wsv_get(eds_win* h, const eds_wsv_out* o) {
    if (int rc = check(h)) return rc;
    if (!o) return fail(EDS_ERR_INVALID, "null output");
    eds_wsv_state* s = h->wsv;
    const int F = s->F, N = 4 + 8 * F;
    const size_t NN = (size_t)N * N, n = (size_t)h->n, m = (size_t)h->m;
    if ((o->HFinal || o->bFinal || o->xAd || o->frame_step) && !s->have_system)
        return fail(EDS_ERR_STATE, "eds_wsv_get: no eds_wsv_solve has run");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    hipStream_t st = h->own.st;
    const double* work = s->work;
#define WSV_GET(dst, src, count) if (o->dst && (count)) EDS_HIP_TRY(hipMemcpyAsync(o->dst, src, (count) * sizeof(*o->dst), hipMemcpyDeviceToHost, st))
    WSV_GET(adHTdeltaF, s->adHTdeltaF, (size_t)F * F * 8);
    WSV_GET(is_linearized, s->lin, m);
    WSV_GET(res_toZeroF, s->rtz, 8 * m);
    WSV_GET(resApprox, s->res_approx, 8 * m);
    WSV_GET(lf, h->lf, 6 * n);
    WSV_GET(HFinal, work + (size_t)edswsv::W_HF * MAX_N * MAX_N, NN);
    WSV_GET(bFinal, work + (size_t)edswsv::W_MATS * MAX_N * MAX_N + (size_t)edswsv::V_BF * MAX_N, (size_t)N);
    WSV_GET(xAd, s->xAd, (size_t)F * F * 8);
    WSV_GET(step, s->step, n);
    WSV_GET(idepth_scaled, h->ids, n);
    WSV_GET(priorF, h->prior, n);
#undef WSV_GET
    EDS_HIP_TRY(hipStreamSynchronize(st));
    if (o->frame_step) for (int i = 0; i < N; ++i) o->frame_step[i] = -s->last_x[i];
    return EDS_OK;
}

}  // extern "C"
