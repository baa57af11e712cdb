// The inverse-depth filter of EDS on the device (include/eds_hip_depth.h): eds::mapping::DepthPoints (reference
// src/mapping/DepthPoints.{hpp,cpp}) for the points of a tracker slot.
//
//   k_depth_init     DepthPoints::init, both overloads (DepthPoints.cpp:59-99), or the seeds as a caller hands them (operator[])
//   k_depth_update   DepthPoints::update (:101-178) in ONE pass per point: keyframe pixel, event-frame pixel (host tracks, host
//                    event-frame coordinates, getCoord's re-projection at the slot's pose, or the KLT's device tracks), triangulation (invDepthTwoPointsEucl,
//                    :368-397), depth uncertainty (computeTau, DepthPoints.hpp:165-182), the Vogiatzis update (filterVogiatzis,
//                    :180-228), the seed write-back and the narrowed mu into the slot's inverse-depth plane
//   k_depth_stats    meanIDepth / medianIDepth (:248-260): fp64 sums and two order statistics by radix select (eds_select.hpp)
//   k_depth_compact  the seeds' share of KeyFrame::erasePoint (KeyFrame.cpp:1060-1106) behind getCoord's compaction (eds_points.hip)
//
// All arithmetic is fp64 and this translation unit is compiled WITHOUT fp contraction (Makefile): every product and sum rounds as
// the reference's does, the transcendentals are OCML's fp64 acos / sin / atan / exp / sqrt.  Each call ends with the slot's plane
// and Gram matrices exactly as eds_trk_set_idepth(mu) leaves them: plane = (float)mu (padding 1.0), eds_gram_kernel's arithmetic
// (eds_launch_gram for one slot, eds_launch_gram_batch for a range).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/eds_hip_depth.h"
#include "eds_capi_internal.hpp"
#include "eds_select.hpp"

using namespace edscapi;
using namespace edssel;

// parameter block of one alignment (doubles, [B][EDS_DP_STRIDE]), filled by the host per launch
#define EDS_DP_PEF 0                // 12  P_ef = K [R | t] of T_ef_kf, row-major 3 x 4 (DepthPoints.cpp:145-148)
#define EDS_DP_KINV 12              // 9   K^-1 (the reference's inv(DECOMP_SVD) of P_kf's 3 x 3 block, :372)
#define EDS_DP_TKE 21               // 3   translation of T_kf_ef (computeTau's t, DepthPoints.hpp:169)
#define EDS_DP_K 24                 // 4   fx fy cx cy
#define EDS_DP_MURANGE 28           // 1   mu_range = max_depth - min_depth
#define EDS_DP_PXERR 29             // 1   px_error_angle
#define EDS_DP_THRESH 30            // 1   convergence_sigma2_thresh
#define EDS_DP_D 31                 // 9   R - I of the slot's pose (re-projection, as eds_points.hip k_update_points)
#define EDS_DP_P 40                 // 3   the slot's translation
#define EDS_DEPTH_TPB 256
#define EDS_DEPTH_SUM 6             // ints per alignment of the summary (eds_depth_summary)
#define EDS_COMPACT_THREADS 1024
#define EDS_COMPACT_PPT 4

namespace {

// init sources beyond the ABI's: the four seed values of every point from the device scratch (operator[] writes)
#define EDS_DEPTH_INIT_SEEDS 3

__device__ __forceinline__ double norm_pdf(double x, double mean, double sigma) {     // Utils.hpp:337-345
    double exponent = x - mean;
    exponent *= -exponent;
    exponent /= 2 * sigma * sigma;
    double result = exp(exponent);
    result /= sigma * sqrt(2 * 3.14159265358979323846);
    return result;
}

__device__ __forceinline__ void count_lanes(bool v, int* dst) {
    const unsigned long long m = __ballot(v);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(dst, __popcll(m));
}

// keyframe pixel the slot holds: integer cell + fp32 fraction (eds_device.hpp), as eds_points.hip reads it
__device__ __forceinline__ void slot_pixel(const EdsArrays& A, size_t o, double& u, double& v) {
    const int c = A.cell0[o];
    u = (double)(short)(c & 0xffff) + (double)A.f0x[o];
    v = (double)(c >> 16) + (double)A.f0y[o];
}

__global__ __launch_bounds__(EDS_DEPTH_TPB) void k_depth_init(EdsArrays A, double* __restrict__ seeds, int first, int nchunk, int source,
                                                            double mu0, double s20, double a0, double b0, const double* __restrict__ in) {
    const int b = blockIdx.x / nchunk, i = (blockIdx.x % nchunk) * EDS_DEPTH_TPB + threadIdx.x;
    const int slot = first + b;
    if (i >= A.Np) return;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const size_t plane = (size_t)A.B * A.Np, o = (size_t)slot * A.Np + i;
    float* rho = const_cast<float*>(A.rho);
    if (i >= N) { rho[o] = 1.f; return; }                     // the padding, as eds_trk_set_idepth leaves it
    const size_t k = (size_t)b * A.Np + i;
    double mu = mu0, s2 = s20, a = a0, bb = b0;
    if (source == EDS_DEPTH_INIT_HOST) mu = in[k];
    else if (source == EDS_DEPTH_INIT_PLANE) mu = (double)A.rho[o];
    else if (source == EDS_DEPTH_INIT_SEEDS) { mu = in[4 * k]; s2 = in[4 * k + 1]; a = in[4 * k + 2]; bb = in[4 * k + 3]; }
    seeds[o] = mu; seeds[plane + o] = s2; seeds[2 * plane + o] = a; seeds[3 * plane + o] = bb;
    rho[o] = (float)mu;
}

// one lane per point; workgroup -> (alignment b, chunk of EDS_DEPTH_TPB points)
__global__ __launch_bounds__(EDS_DEPTH_TPB) void k_depth_update(EdsArrays A, double* __restrict__ seeds, const double* __restrict__ par, int first,
                                                              int nchunk, int coords, const double* __restrict__ xy,
                                                              const double* __restrict__ kfxy, const double* __restrict__ tpl,
                                                              int* __restrict__ sum) {
    const int b = blockIdx.x / nchunk, i = (blockIdx.x % nchunk) * EDS_DEPTH_TPB + threadIdx.x;
    const int slot = first + b;
    if (i >= A.Np) return;              // (uniform per wavefront: Np is a multiple of 64)
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const double* __restrict__ P = par + (size_t)b * EDS_DP_STRIDE;
    const size_t plane = (size_t)A.B * A.Np, o = (size_t)slot * A.Np + i, k = (size_t)b * A.Np + i;
    float* rho_plane = const_cast<float*>(A.rho);
    bool updated = false, skipped = false, restored = false, reset = false, converged = false;
    if (i < N) {
        const double fx = P[EDS_DP_K], fy = P[EDS_DP_K + 1], cx = P[EDS_DP_K + 2], cy = P[EDS_DP_K + 3];
        // keyframe pixel, event-frame pixel
        double ukf, vkf;
        if (kfxy) { ukf = kfxy[2 * k]; vkf = kfxy[2 * k + 1]; }
        else slot_pixel(A, o, ukf, vkf);
        double uef, vef;
        if (coords == EDS_DEPTH_EF_COORD) { uef = xy[2 * k]; vef = xy[2 * k + 1]; }
        else if (coords == EDS_DEPTH_TRACKS) { uef = ukf + xy[2 * k]; vef = vkf + xy[2 * k + 1]; }
        else if (coords == EDS_DEPTH_DEVICE_TRACKS) { uef = ukf + tpl[o]; vef = vkf + tpl[plane + o]; }      // the KLT's kf->tracks
        else {
            // Tracker::getCoord's track at the slot's pose with the raw inverse depth (Tracker.cpp:343-351; k_update_points' expression)
            const double x = (double)A.x[o], y = (double)A.y[o], r = (double)A.rho[o];
            const double* D = P + EDS_DP_D;
            const double d0 = D[0] * x + D[1] * y + D[2] + P[EDS_DP_P] * r;
            const double d1 = D[3] * x + D[4] * y + D[5] + P[EDS_DP_P + 1] * r;
            const double d2 = D[6] * x + D[7] * y + D[8] + P[EDS_DP_P + 2] * r;
            const double is = 1.0 / (1.0 + d2);
            uef = ukf + fx * (d0 - x * d2) * is;
            vef = vkf + fy * (d1 - y * d2) * is;
        }
        // invDepthTwoPointsEucl (DepthPoints.cpp:368-397): x1p = M2 (M1^-1 x_kf), e2 = P_ef (0, 0, 0, 1), inv = (x1p x x_ef).(x_ef x e2) / |x_ef x e2|^2
        const double* Ki = P + EDS_DP_KINV;
        const double* Pe = P + EDS_DP_PEF;
        const double y0 = Ki[0] * ukf + Ki[1] * vkf + Ki[2];
        const double y1 = Ki[3] * ukf + Ki[4] * vkf + Ki[5];
        const double y2 = Ki[6] * ukf + Ki[7] * vkf + Ki[8];
        const double p0 = Pe[0] * y0 + Pe[1] * y1 + Pe[2] * y2;
        const double p1 = Pe[4] * y0 + Pe[5] * y1 + Pe[6] * y2;
        const double p2 = Pe[8] * y0 + Pe[9] * y1 + Pe[10] * y2;
        const double e0 = Pe[3], e1 = Pe[7], e2 = Pe[11];
        const double a1x = p1 * 1.0 - p2 * vef, a1y = p2 * uef - p0 * 1.0, a1z = p0 * vef - p1 * uef;
        const double a2x = vef * e2 - 1.0 * e1, a2y = 1.0 * e0 - uef * e2, a2z = uef * e1 - vef * e0;
        const double inv_depth = (a1x * a2x + a1y * a2y + a1z * a2z) / (a2x * a2x + a2y * a2y + a2z * a2z);
        const double depth = 1.0 / inv_depth;
        // computeTau (DepthPoints.hpp:165-182): t of T_kf_ef, bearing of the EVENT-frame pixel
        const double xn = (uef - cx) / fx, yn = (vef - cy) / fy;
        const double bn = sqrt(xn * xn + yn * yn + 1.0 * 1.0);
        const double bx = xn / bn, by = yn / bn, bz = 1.0 / bn;
        const double tx = P[EDS_DP_TKE], ty = P[EDS_DP_TKE + 1], tz = P[EDS_DP_TKE + 2];
        const double ax = bx * depth - tx, ay = by * depth - ty, az = bz * depth - tz;
        const double t_norm = sqrt(tx * tx + ty * ty + tz * tz);
        const double a_norm = sqrt(ax * ax + ay * ay + az * az);
        const double alpha = acos((bx * tx + by * ty + bz * tz) / t_norm);
        const double beta = acos((ax * -tx + ay * -ty + az * -tz) / (t_norm * a_norm));
        const double beta_plus = beta + P[EDS_DP_PXERR];
        const double gamma_plus = 3.14159265358979323846 - alpha - beta_plus;
        const double z_plus = t_norm * sin(beta_plus) / sin(gamma_plus);
        const double tau = z_plus - depth;
        // getSigma2FromDepthSigma (:184-189): std::max(1e-12, d) is (1e-12 < d) ? d : 1e-12
        const double dm = depth - tau;
        const double sg = 0.5 * (1.0 / ((1e-12 < dm) ? dm : 1e-12) - 1.0 / (depth + tau));
        const double tau2 = sg * sg;
        // filterVogiatzis (DepthPoints.cpp:180-228), literally
        const double mu_range = P[EDS_DP_MURANGE];
        double mu = seeds[o], sigma2 = seeds[plane + o], a = seeds[2 * plane + o], bb = seeds[3 * plane + o];
        const double norm_scale = sqrt(sigma2 + tau2);
        if (isnan(norm_scale)) {
            skipped = true;
        } else {
            updated = true;
            const double z = inv_depth;
            const double oldsigma2 = sigma2;
            const double s2 = 1.0 / (1.0 / sigma2 + 1.0 / tau2);
            const double m = s2 * (mu / sigma2 + z / tau2);
            const double uniform_x = 1.0 / mu_range;
            double C1 = a / (a + bb) * norm_pdf(z, mu, norm_scale);
            double C2 = bb / (a + bb) * uniform_x;
            const double normalization_constant = C1 + C2;
            C1 /= normalization_constant;
            C2 /= normalization_constant;
            const double f = C1 * (a + 1.0) / (a + bb + 1.0) + C2 * a / (a + bb + 1.0);
            const double e = C1 * (a + 1.0) * (a + 2.0) / ((a + bb + 1.0) * (a + bb + 2.0)) + C2 * a * (a + 1.0) / ((a + bb + 1.0) * (a + bb + 2.0));
            const double mu_new = C1 * m + C2 * mu;
            sigma2 = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu_new * mu_new;
            mu = mu_new;
            a = (e - f) / (f - e / f);
            bb = a * (1.0 - f) / f;
            if (sigma2 < 0.0) { restored = true; sigma2 = oldsigma2; }
            if (mu < 0.0) { reset = true; mu = 1.0; }
            seeds[o] = mu; seeds[plane + o] = sigma2; seeds[2 * plane + o] = a; seeds[3 * plane + o] = bb;
        }
        const double thresh = mu_range / P[EDS_DP_THRESH];         // isConverged (DepthPoints.hpp:183-193)
        converged = sigma2 < thresh * thresh;
        rho_plane[o] = (float)mu;
    } else {
        rho_plane[o] = 1.f;
    }
    int* s = sum + (size_t)b * EDS_DEPTH_SUM;
    count_lanes(updated, s); count_lanes(skipped, s + 1); count_lanes(restored, s + 2); count_lanes(reset, s + 3); count_lanes(converged, s + 4);
}

// out[4 b ..] = mean, variance (n - 1; 0 for n = 1), value at sorted position n/2, at n/3 — one workgroup per alignment
__global__ __launch_bounds__(EDS_LP_THREADS) void k_depth_stats(EdsArrays A, const double* __restrict__ seeds, int first, double* __restrict__ out) {
    const int slot = first + blockIdx.x, tid = threadIdx.x;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const double* __restrict__ mu = seeds + (size_t)slot * A.Np;
    out += 4 * (size_t)blockIdx.x;
    __shared__ double s_part[EDS_LP_THREADS / 64];
    __shared__ double s_bcast;
    __shared__ int s_hist[256], s_cnt[2];
    __shared__ unsigned long long s_sel[1];
    // mean_std_vector (Utils.hpp:272-290): the "std_dev" it returns is the variance
    double acc = 0.0;
    for (int i = tid; i < N; i += EDS_LP_THREADS) acc += mu[i];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) { double t = 0; for (int w = 0; w < EDS_LP_THREADS / 64; ++w) t += s_part[w]; s_bcast = N == 1 ? mu[0] : t / (double)N; }
    __syncthreads();
    const double mean = s_bcast;
    acc = 0.0;
    if (N > 1)
        for (int i = tid; i < N; i += EDS_LP_THREADS) { const double d = mu[i] - mean; acc += d * d / (double)(N - 1); }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) { double t = 0; for (int w = 0; w < EDS_LP_THREADS / 64; ++w) t += s_part[w]; out[0] = mean; out[1] = t; }
    // n_quantile_vector (Utils.hpp:315-320) at n/2 and n/3: order statistics, nothing is sorted
    const double median = val_of(radix_select([&](int i) { return key_of(mu[i]); }, N, N / 2, tid, s_hist, s_sel, s_cnt));
    const double third = val_of(radix_select([&](int i) { return key_of(mu[i]); }, N, N / 3, tid, s_hist, s_sel, s_cnt));
    if (tid == 0) { out[2] = median; out[3] = third; }
}

// seeds[dst] = seeds[kept[dst]] for dst < the slot's new N (k_update_points has just written both).  kept[dst] >= dst: a sweep reads
// all its sources before it writes, and a later sweep's sources lie beyond every earlier sweep's destinations — in place, in order.
__global__ __launch_bounds__(EDS_COMPACT_THREADS) void k_depth_compact(EdsArrays A, double* __restrict__ seeds, int first,
                                                                     const int* __restrict__ kept) {
    const int slot = first + blockIdx.x, tid = threadIdx.x;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const size_t plane = (size_t)A.B * A.Np, base = (size_t)slot * A.Np;
    kept += (size_t)A.Np * blockIdx.x;
    for (int c0 = 0; c0 < N; c0 += EDS_COMPACT_THREADS * EDS_COMPACT_PPT) {
        double v[EDS_COMPACT_PPT][4];
#pragma unroll
        for (int j = 0; j < EDS_COMPACT_PPT; ++j) {
            const int d = c0 + j * EDS_COMPACT_THREADS + tid;
            if (d < N) {
                const size_t src = base + kept[d];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[j][c] = seeds[c * plane + src];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EDS_COMPACT_PPT; ++j) {
            const int d = c0 + j * EDS_COMPACT_THREADS + tid;
            if (d < N)
#pragma unroll
                for (int c = 0; c < 4; ++c) seeds[c * plane + base + d] = v[j][c];
        }
        __syncthreads();
    }
}

int ensure(eds_trk* h) {
    EdsDepthBuffers& d = h->depth;
    if (d.seeds) return EDS_OK;
    const size_t B = (size_t)h->B, Np = (size_t)h->Np;
    if (!h->own.alloc({{(void**)&d.seeds, 4 * B * Np * 8}, {(void**)&d.d_par, B * EDS_DP_STRIDE * 8}, {(void**)&d.d_sum, B * EDS_DEPTH_SUM * 4},
                       {(void**)&d.d_stats, B * 4 * 8}, pinned(d.h_par, B * EDS_DP_STRIDE * 8), pinned(d.h_sum, B * EDS_DEPTH_SUM * 4),
                       pinned(d.h_stats, B * 4 * 8)}))
        return fail(EDS_ERR_HIP, "allocation of the depth-filter buffers failed");
    return EDS_OK;
}

int ensure_input(eds_trk* h) {
    EdsDepthBuffers& d = h->depth;
    if (d.d_in) return EDS_OK;
    if (!h->own.alloc(d.d_in, 4 * (size_t)h->B * h->Np * 8)) return fail(EDS_ERR_HIP, "allocation of the depth-filter input buffer failed");
    return EDS_OK;
}

// rows b = 0 .. count - 1 of `width` doubles per point: src[(b * stride + i) * width] -> dst[(b * Np + i) * width] for i < N(first + b).
// One 2-D copy for all rows but the last (a row never reads past the next row's start), the last row by its own length.
int upload_rows(eds_trk* h, int first, int count, const double* src, int stride, int width, double* dst) {
    const size_t Np = (size_t)h->Np, w = (size_t)width * 8;
    const size_t row = (size_t)std::min(stride, h->Np) * w;
    if (count > 1)
        EDS_HIP_TRY(hipMemcpy2DAsync(dst, Np * w, src, (size_t)stride * w, row, (size_t)count - 1, hipMemcpyHostToDevice, h->own.st));
    const int nl = h->slots[first + count - 1].N;
    EDS_HIP_TRY(hipMemcpyAsync(dst + (size_t)(count - 1) * Np * width, src + (size_t)(count - 1) * stride * width, (size_t)nl * w,
                               hipMemcpyHostToDevice, h->own.st));
    return EDS_OK;
}

// the slots' planes were just written: Gram matrices as eds_trk_set_idepth refreshes them, on the device only (fill_pose fetches h_G
// for a host-side reader); the caller waits for the stream
int finish_planes(eds_trk* h, int first, int count) {
    const int nb = effective_blocks(h);
    if (count == 1) eds_launch_gram(h->arrays(), first, nb, h->own.st);
    else eds_launch_gram_batch(h->arrays(), first, count, nb, h->own.st);
    EDS_HIP_TRY(hipGetLastError());
    for (int s = first; s < first + count; ++s) h->slots[s].gram_host_stale = true;
    return EDS_OK;
}

int launch_init(eds_trk* h, int first, int count, int source, double mu0, double s20, double a0, double b0, const double* in) {
    const int nchunk = (h->Np + EDS_DEPTH_TPB - 1) / EDS_DEPTH_TPB;
    hipLaunchKernelGGL(k_depth_init, dim3((unsigned)count * nchunk), dim3(EDS_DEPTH_TPB), 0, h->own.st, h->arrays(), h->depth.seeds, first, nchunk,
                       source, mu0, s20, a0, b0, in);
    EDS_HIP_TRY(hipGetLastError());
    int rc = finish_planes(h, first, count);
    if (rc) return rc;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int read_plane(eds_trk* h, int slot, int c, double* dst) {
    EDS_HIP_TRY(hipMemcpyAsync(dst, h->depth.seeds + (size_t)c * h->B * h->Np + (size_t)slot * h->Np, (size_t)h->slots[slot].N * 8,
                               hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

}  // namespace

void eds_depth_compact(eds_trk* h, int first, int count, const int* kept) {
    if (!h->depth.seeds) return;
    hipLaunchKernelGGL(k_depth_compact, dim3(count), dim3(EDS_COMPACT_THREADS), 0, h->own.st, h->arrays(), h->depth.seeds, first, kept);
}

extern "C" {

int eds_depth_abi_version(void) { return EDS_HIP_DEPTH_ABI_VERSION; }

void eds_depth_params_default(eds_depth_params* prm) {
    if (!prm) return;
    prm->min_depth = 1.0; prm->max_depth = 3.0;         // eds_kf_select_default's range
    prm->threshold = 100.0; prm->init_a = 2.0; prm->init_b = 5.0;      // DepthPoints.hpp:60-61
}

int eds_depth_init(eds_trk* h, int first, int count, const eds_depth_params* prm, int source, const double* idp, int stride) {
    int rc = check_range(h, first, count);
    if (rc || (rc = check_idle_slots(h, first, count, EDS_NEED_KF))) return rc;
    if (!prm) return fail(EDS_ERR_INVALID, "null parameters");
    if (source < EDS_DEPTH_INIT_CONSTANT || source > EDS_DEPTH_INIT_PLANE) return fail(EDS_ERR_INVALID, "unknown init source");
    if (source == EDS_DEPTH_INIT_HOST) {
        if (!idp) return fail(EDS_ERR_INVALID, "null inverse depths");
        if (stride < max_points(h, first, count)) return fail(EDS_ERR_INVALID, "stride smaller than the largest point count");
    }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = ensure(h))) return rc;
    if (source == EDS_DEPTH_INIT_HOST && ((rc = ensure_input(h)) || (rc = upload_rows(h, first, count, idp, stride, 1, h->depth.d_in)))) return rc;
    const double mu_range = prm->max_depth - prm->min_depth;
    const double mu0 = 1.0 / ((prm->max_depth - prm->min_depth) / 2.0);
    const double s20 = source == EDS_DEPTH_INIT_CONSTANT ? mu_range * mu_range : (mu_range * mu_range) / 36.0;
    if ((rc = launch_init(h, first, count, source, mu0, s20, prm->init_a, prm->init_b, h->depth.d_in))) return rc;
    for (int s = first; s < first + count; ++s) {
        Slot& sl = h->slots[s];
        sl.seeded = true;
        sl.dp_mu_range = mu_range;
        sl.dp_px_error_angle = std::atan(3.0 / (2.0 * sl.K[0])) + std::atan(3.0 / (2.0 * sl.K[1]));    // getAngleError(px_noise = 3)
        sl.dp_threshold = prm->threshold;
    }
    return EDS_OK;
}

int eds_depth_update(eds_trk* h, int first, int count, int coords, const double* xy, const double* kf_xy, int stride, const double* T_kf_ef,
                     int filter, eds_depth_summary* out) {
    return eds_depth_update_impl(h, first, count, coords, xy, kf_xy, stride, T_kf_ef, filter, out, nullptr);
}

}  // extern "C"

int eds_depth_update_impl(eds_trk* h, int first, int count, int coords, const double* xy, const double* kf_xy, int stride,
                          const double* T_kf_ef, int filter, eds_depth_summary* out, const double* dev_ef) {
    int rc = check_range(h, first, count);
    if (rc || (rc = check_idle_slots(h, first, count, EDS_NEED_KF | EDS_NEED_SEEDS))) return rc;
    if (coords < EDS_DEPTH_TRACKS || coords > EDS_DEPTH_DEVICE_TRACKS) return fail(EDS_ERR_INVALID, "unknown coordinate source");
    if (filter != EDS_DEPTH_VOGIATZIS && filter != EDS_DEPTH_GAUSS) return fail(EDS_ERR_INVALID, "unknown depth filter");
    const bool on_device = coords == EDS_DEPTH_REPROJECT || coords == EDS_DEPTH_DEVICE_TRACKS;
    if (!xy && !dev_ef && !on_device) return fail(EDS_ERR_INVALID, "null event-frame coordinates");
    if (on_device) xy = nullptr;
    if ((xy || kf_xy) && stride < max_points(h, first, count)) return fail(EDS_ERR_INVALID, "stride smaller than the largest point count");
    if (coords == EDS_DEPTH_DEVICE_TRACKS && !h->klt.tracks)
        return fail(EDS_ERR_STATE, "no device tracks: eds_klt_track_points has not run on this handle (include/eds_hip_klt.h)");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EdsDepthBuffers& d = h->depth;
    const size_t half = 2 * (size_t)h->B * h->Np;
    if (xy || kf_xy) {
        if ((rc = ensure_input(h))) return rc;
        if (xy && (rc = upload_rows(h, first, count, xy, stride, 2, d.d_in))) return rc;
        if (kf_xy && (rc = upload_rows(h, first, count, kf_xy, stride, 2, d.d_in + half))) return rc;
    }
    for (int b = 0; b < count; ++b) {
        const Slot& s = h->slots[first + b];
        double* P = d.h_par + (size_t)b * EDS_DP_STRIDE;
        // T_ef_kf = T_kf_ef^-1 (DepthPoints.cpp:145): the slot's pose itself, or the inverse of the caller's T_kf_ef
        double R[9], t[3];
        if (T_kf_ef) {
            const double* T = T_kf_ef + 7 * (size_t)b;
            double Rk[9];
            edsm::quat_to_R(T + 3, Rk);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) R[3 * r + c] = Rk[3 * c + r];
            for (int r = 0; r < 3; ++r) t[r] = -(R[3 * r] * T[0] + R[3 * r + 1] * T[1] + R[3 * r + 2] * T[2]);
            for (int r = 0; r < 3; ++r) P[EDS_DP_TKE + r] = T[r];
        } else {
            edsm::quat_to_R(s.q, R);
            for (int r = 0; r < 3; ++r) t[r] = s.p[r];
            for (int r = 0; r < 3; ++r) P[EDS_DP_TKE + r] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);       // -R^T p
        }
        const double fx = s.K[0], fy = s.K[1], cx = s.K[2], cy = s.K[3];
        const double K[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
        for (int r = 0; r < 3; ++r) {               // P_ef = K [R | t]
            for (int c = 0; c < 3; ++c) P[EDS_DP_PEF + 4 * r + c] = K[3 * r] * R[c] + K[3 * r + 1] * R[3 + c] + K[3 * r + 2] * R[6 + c];
            P[EDS_DP_PEF + 4 * r + 3] = K[3 * r] * t[0] + K[3 * r + 1] * t[1] + K[3 * r + 2] * t[2];
        }
        const double Ki[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
        for (int j = 0; j < 9; ++j) P[EDS_DP_KINV + j] = Ki[j];
        for (int j = 0; j < 4; ++j) P[EDS_DP_K + j] = s.K[j];
        P[EDS_DP_MURANGE] = s.dp_mu_range; P[EDS_DP_PXERR] = s.dp_px_error_angle; P[EDS_DP_THRESH] = s.dp_threshold;
        edsm::quat_to_RmI(s.q, P + EDS_DP_D);       // getCoord's pose (eds_points.hip)
        for (int r = 0; r < 3; ++r) P[EDS_DP_P + r] = s.p[r];
    }
    EDS_HIP_TRY(hipMemcpyAsync(d.d_par, d.h_par, (size_t)count * EDS_DP_STRIDE * 8, hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(d.d_sum, 0, (size_t)count * EDS_DEPTH_SUM * 4, h->own.st));
    const int nchunk = (h->Np + EDS_DEPTH_TPB - 1) / EDS_DEPTH_TPB;
    hipLaunchKernelGGL(k_depth_update, dim3((unsigned)count * nchunk), dim3(EDS_DEPTH_TPB), 0, h->own.st, h->arrays(), d.seeds, d.d_par, first, nchunk,
                       coords, dev_ef ? dev_ef : (xy ? d.d_in : nullptr), kf_xy ? d.d_in + half : nullptr, h->klt.tracks, d.d_sum);
    EDS_HIP_TRY(hipGetLastError());
    if ((rc = finish_planes(h, first, count))) return rc;
    EDS_HIP_TRY(hipMemcpyAsync(d.h_sum, d.d_sum, (size_t)count * EDS_DEPTH_SUM * 4, hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    if (out) std::memcpy(out, d.h_sum, (size_t)count * sizeof(eds_depth_summary));
    return EDS_OK;
}

extern "C" {

int eds_depth_get(eds_trk* h, int slot, double* mu_s2_a_b, uint8_t* converged) {
    int rc = check_range(h, slot, 1);
    if (rc || (rc = check_idle_slots(h, slot, 1, EDS_NEED_KF | EDS_NEED_SEEDS))) return rc;
    if (!mu_s2_a_b && !converged) return fail(EDS_ERR_INVALID, "null output");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const Slot& s = h->slots[slot];
    const size_t N = (size_t)s.N;
    std::vector<double> v(4 * N);
    for (int c = 0; c < 4; ++c)
        if ((rc = read_plane(h, slot, c, v.data() + c * N))) return rc;
    const double thresh = s.dp_mu_range / s.dp_threshold;
    for (size_t i = 0; i < N; ++i) {
        if (mu_s2_a_b)
            for (int c = 0; c < 4; ++c) mu_s2_a_b[4 * i + c] = v[c * N + i];
        if (converged) converged[i] = v[N + i] < thresh * thresh;
    }
    return EDS_OK;
}

int eds_depth_set(eds_trk* h, int slot, const double* mu_s2_a_b) {
    int rc = check_range(h, slot, 1);
    if (rc || (rc = check_idle_slots(h, slot, 1, EDS_NEED_KF | EDS_NEED_SEEDS))) return rc;
    if (!mu_s2_a_b) return fail(EDS_ERR_INVALID, "null seeds");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = ensure_input(h))) return rc;
    EDS_HIP_TRY(hipMemcpyAsync(h->depth.d_in, mu_s2_a_b, (size_t)h->slots[slot].N * 32, hipMemcpyHostToDevice, h->own.st));
    return launch_init(h, slot, 1, EDS_DEPTH_INIT_SEEDS, 0.0, 0.0, 0.0, 0.0, h->depth.d_in);
}

int eds_depth_get_idepth(eds_trk* h, int slot, double* mu) {
    int rc = check_range(h, slot, 1);
    if (rc || (rc = check_idle_slots(h, slot, 1, EDS_NEED_KF | EDS_NEED_SEEDS))) return rc;
    if (!mu) return fail(EDS_ERR_INVALID, "null output");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    return read_plane(h, slot, 0, mu);
}

int eds_depth_stats(eds_trk* h, int first, int count, double* out4) {
    int rc = check_range(h, first, count);
    if (rc || (rc = check_idle_slots(h, first, count, EDS_NEED_KF | EDS_NEED_SEEDS))) return rc;
    if (!out4) return fail(EDS_ERR_INVALID, "null output");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EdsDepthBuffers& d = h->depth;
    hipLaunchKernelGGL(k_depth_stats, dim3(count), dim3(EDS_LP_THREADS), 0, h->own.st, h->arrays(), d.seeds, first, d.d_stats);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipMemcpyAsync(d.h_stats, d.d_stats, (size_t)count * 32, hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    std::memcpy(out4, d.h_stats, (size_t)count * 32);
    return EDS_OK;
}

}  // extern "C"
