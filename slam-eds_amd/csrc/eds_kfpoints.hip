// What KeyFrame does to its own point set, on the device (include/eds_hip_kfpoints.h), for the points of a tracker slot:
//
//   k_kfp_range     KeyFrame::pointsRefinement (reference src/tracking/KeyFrame.cpp:1031-1058): one wavefront per point, max - min of the
//                   (2r+1)^2 window of the event frame at the TRUNCATED keyframe pixel, and the erase flag |max - min| < event_diff.
//                   A window wholly inside a tiled frame is read tile by tile: one lane per 4 x 4 tile (64 bytes, four 16-byte loads),
//                   the taps outside the window masked; 23 x 23 spans at most 7 x 7 tiles, one pass.  Any other window (one that
//                   touches the border, a row-major frame) goes tap by tap through border_map, as k_epi_templates reads the model.
//   k_kfp_clean     KeyFrame::cleanPoints (:1566-1587): the erase flag weight < threshold
//   then getCoord's compaction (k_update_points, eds_points.hip) erases by flag, with the seeds and the KLT's tracks and flow — the
//   path of the epiline cull (eds_epiline.hip), so a slot ends exactly as that cull leaves it.
//   k_kfp_project   getDepthMap() (:1220-1237) -> T_dst_src -> IDepthMap::fromPoints (src/mapping/Types.hpp:248-275): one workgroup per
//                   alignment, sweeps of 1024 points, a ballot scan for order-preserving destinations, outputs in mapped pinned memory.
//
// min / max are exact and the projection is fp64 without FMA contraction (this translation unit is compiled with -ffp-contract=off,
// Makefile); every result has a fixed order, so a batch equals its singles bit for bit and runs repeat exactly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <tuple>
#include <vector>

#include "../../include/eds_hip_kfpoints.h"
#include "eds_capi_internal.hpp"
#include "eds_device.hpp"
#include "eds_splat.hpp"

using namespace edscapi;
using namespace edsd;
using namespace edssplat;

#define EDS_KFP_MAX_RADIUS 15
#define EDS_KFP_WAVES 4             // points per workgroup of k_kfp_range
#define EDS_KFP_PROJ_THREADS 1024
#define EDS_KFP_TRUNC_MAX 1048576.0 // a truncated pixel coordinate beyond +-2^20 is taken as +-2^20

namespace {

// cv::Rect of a Point2d: the coordinate TRUNCATED (k_epi_templates' rule on cell + fp32 fraction)
__device__ __forceinline__ int trunc_pixel(double u) { return (int)fmin(fmax(u, -EDS_KFP_TRUNC_MAX), EDS_KFP_TRUNC_MAX); }

// point i = blockIdx.x * EDS_KFP_WAVES + wavefront of alignment blockIdx.y (slot first + blockIdx.y)
__global__ __launch_bounds__(64 * EDS_KFP_WAVES) void k_kfp_range(EdsArrays A, int first, int r, int border, float bval, double event_diff,
                                                                  double* __restrict__ range, unsigned char* __restrict__ erase) {
    const int slot = first + blockIdx.y, lane = threadIdx.x & 63, H = A.H, W = A.W;
    const int i = blockIdx.x * EDS_KFP_WAVES + (threadIdx.x >> 6);
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (i >= N) return;
    const size_t o = (size_t)slot * A.Np + i;
    const int c = A.cell0[o];
    const int tx = trunc_pixel((double)(short)(c & 0xffff) + (double)A.f0x[o]), ty = trunc_pixel((double)(c >> 16) + (double)A.f0y[o]);
    const FrameView fv = make_frame_view(A.frame, (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_FRAME], H, W, A.Hp, A.Wp, A.tiled);
    const int x0 = tx - r, x1 = tx + r, y0 = ty - r, y1 = ty + r;
    float lo = __builtin_nanf(""), hi = __builtin_nanf("");       // fminf / fmaxf return the other operand of a NaN
    if (A.tiled && x0 >= 0 && y0 >= 0 && x1 < W && y1 < H) {
        const int tc0 = x0 >> 2, tr0 = y0 >> 2, ntx = (x1 >> 2) - tc0 + 1, nty = (y1 >> 2) - tr0 + 1;
        for (int t = lane; t < ntx * nty; t += 64) {
            const int jr = t / ntx, tr = tr0 + jr, tc = tc0 + (t - jr * ntx);
            // tile (tr, tc): logical rows 4 tr .. 4 tr + 3 < H <= the allocation, 16 floats at a 64-byte boundary
            const float4* __restrict__ T = reinterpret_cast<const float4*>(fv.base + frame_index(fv, 4 * tr, 4 * tc));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 q = T[j];
                const int y = 4 * tr + j, x = 4 * tc;
                if (y < y0 || y > y1) continue;
                if (x >= x0 && x <= x1) { lo = fminf(lo, q.x); hi = fmaxf(hi, q.x); }
                if (x + 1 >= x0 && x + 1 <= x1) { lo = fminf(lo, q.y); hi = fmaxf(hi, q.y); }
                if (x + 2 >= x0 && x + 2 <= x1) { lo = fminf(lo, q.z); hi = fmaxf(hi, q.z); }
                if (x + 3 >= x0 && x + 3 <= x1) { lo = fminf(lo, q.w); hi = fmaxf(hi, q.w); }
            }
        }
    } else {
        const int S = 2 * r + 1, K = S * S;
        for (int j = lane; j < K; j += 64) {
            const int ky = j / S, kx = j - ky * S;
            const int my = y0 + ky, mx = x0 + kx;
            float v;
            if (border == EDS_EPI_BORDER_CONSTANT && ((unsigned)my >= (unsigned)H || (unsigned)mx >= (unsigned)W)) v = bval;
            else v = fv.base[frame_index(fv, border_map(my, H, border), border_map(mx, W, border))];
            lo = fminf(lo, v); hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if (lane == 0) {
        const double d = fabs((double)hi - (double)lo);           // KeyFrame.cpp:1048
        range[o] = d;
        erase[o] = d < event_diff ? 1 : 0;                         // a NaN range (no finite tap) is kept
    }
}

__global__ __launch_bounds__(256) void k_kfp_clean(EdsArrays A, int first, double thr, unsigned char* __restrict__ erase) {
    const int slot = first + blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (i >= N) return;
    const size_t o = (size_t)slot * A.Np + i;
    erase[o] = (double)A.w[o] < thr ? 1 : 0;                        // KeyFrame.cpp:1572
}

// One workgroup per alignment b = blockIdx.x (slot first + b); par, n_out, xy, idp, src at their b-th places (mapped pinned memory)
__global__ __launch_bounds__(EDS_KFP_PROJ_THREADS) void k_kfp_project(EdsArrays A, int first, const double* __restrict__ par,
                                                                      const double* __restrict__ seeds_mu, int* __restrict__ n_out,
                                                                      double* __restrict__ xy, double* __restrict__ idp_out,
                                                                      int* __restrict__ src) {
    __shared__ double s_par[EDS_KFP_PAR];
    __shared__ int s_wave[EDS_KFP_PROJ_THREADS / 64];
    const int b = blockIdx.x, slot = first + b, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (tid < EDS_KFP_PAR) s_par[tid] = par[(size_t)b * EDS_KFP_PAR + tid];
    __syncthreads();
    const double* R = s_par;
    const double t0 = s_par[9], t1 = s_par[10], t2 = s_par[11];
    const double fx = s_par[12], fy = s_par[13], cx = s_par[14], cy = s_par[15];
    const double fxd = s_par[16], fyd = s_par[17], cxd = s_par[18], cyd = s_par[19];
    const double dW = s_par[20], dH = s_par[21];
    const bool seeded = s_par[22] != 0.0;
    const size_t base = (size_t)slot * A.Np, ob = (size_t)b * A.Np;
    int run = 0;
    for (int c0 = 0; c0 < N; c0 += EDS_KFP_PROJ_THREADS) {
        const int i = c0 + tid;
        bool keep = false;
        double px = 0.0, py = 0.0, ip = 0.0;
        if (i < N) {
            const size_t o = base + i;
            const int c = A.cell0[o];
            const double u = (double)(short)(c & 0xffff) + (double)A.f0x[o], v = (double)(c >> 16) + (double)A.f0y[o];
            const double mu = seeded ? seeds_mu[o] : (double)A.rho[o];
            const double d = 1.0 / mu;                                          // getDepthMap (KeyFrame.cpp:1226-1233)
            const double X = d * ((u - cx) / fx), Y = d * ((v - cy) / fy), Z = d;
            const double Xp = R[0] * X + R[1] * Y + R[2] * Z + t0;
            const double Yp = R[3] * X + R[4] * Y + R[5] * Z + t1;
            const double Zp = R[6] * X + R[7] * Y + R[8] * Z + t2;
            px = fxd * (Xp / Zp) + cxd; py = fyd * (Yp / Zp) + cyd;             // IDepthMap::fromPoints (Types.hpp:256-266)
            ip = 1.0 / Zp;
            keep = px >= 0.0 && px < dW && py >= 0.0 && py < dH;                // a NaN fails; Z' <= 0 is not tested, as there
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < EDS_KFP_PROJ_THREADS / 64; ++w) { const int n = s_wave[w]; before += w < wave ? n : 0; total += n; }
        if (keep) {
            const size_t dst = ob + (size_t)(run + before + __popcll(m & ((1ull << lane) - 1ull)));
            xy[2 * dst] = px; xy[2 * dst + 1] = py;
            idp_out[dst] = ip;
            src[dst] = i;
        }
        run += total;
        __syncthreads();
    }
    if (tid == 0) n_out[b] = run;
}

int ensure_flags(eds_trk* h) {
    EdsKfpBuffers& k = h->kfp;
    if (k.erase) return EDS_OK;
    const size_t B = (size_t)h->B, Np = (size_t)h->Np;
    if (!h->own.alloc({{(void**)&k.range, B * Np * 8}, {(void**)&k.erase, B * Np}, {(void**)&k.coord, 2 * B * Np * 8}, {(void**)&k.kept, B * Np * 4}}))
        return fail(EDS_ERR_HIP, "allocation of the keyframe point buffers failed");
    return EDS_OK;
}

int ensure_project(eds_trk* h, int cap) {
    EdsKfpBuffers& k = h->kfp;
    if (k.h_block && k.cap >= cap) return EDS_OK;
    const size_t Np = (size_t)h->Np;
    const size_t bytes = (size_t)cap * (EDS_KFP_PAR * 8 + 8 + Np * 16 + Np * 8 + Np * 4);      // par | n (padded to 8) | xy | idp | src
    char* dblock = nullptr;
    if (!h->own.regrow(k.cap, cap, {mapped(k.h_block, dblock, bytes)})) return fail(EDS_ERR_HIP, "allocation of the projection buffers failed");
    auto carve = [&](char* base) {
        double* par = reinterpret_cast<double*>(base);
        double* xy = par + (size_t)EDS_KFP_PAR * cap;
        double* idp = xy + 2 * Np * cap;
        int* n = reinterpret_cast<int*>(idp + Np * cap);
        int* src = n + 2 * (size_t)cap;
        return std::make_tuple(par, xy, idp, n, src);
    };
    std::tie(k.h_par, k.h_xy, k.h_idp, k.h_n, k.h_src) = carve(k.h_block);
    std::tie(k.d_par, k.d_xy, k.d_idp, k.d_n, k.d_src) = carve(dblock);
    return EDS_OK;
}

bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
    return true;
}

// The slots' flags are in kfp.erase: erase by flag (erase_now), then the kept indices and counts.  n0: the point counts before
int finish_erase(eds_trk* h, int first, int count, bool erase_now, int stride, int32_t* kept_index, int* n_kept) {
    EdsKfpBuffers& k = h->kfp;
    const size_t Np = (size_t)h->Np;
    int rc;
    if (erase_now) {
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
        const EdsPointsDev dev = {k.coord, k.kept, k.erase};
        if ((rc = update_points_range(h, first, count, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &dev))) return rc;
    }
    std::vector<int32_t> vk;
    if (kept_index && erase_now) { vk.resize(Np * count); EDS_HIP_TRY(hipMemcpyAsync(vk.data(), k.kept + Np * first, Np * count * 4, hipMemcpyDeviceToHost, h->own.st)); }
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    for (int b = 0; b < count; ++b) {
        const int nk = h->slots[first + b].N;
        if (n_kept) n_kept[b] = nk;
        for (int q = 0; kept_index && q < nk; ++q) kept_index[(size_t)b * stride + q] = erase_now ? vk[Np * b + q] : q;
    }
    return EDS_OK;
}

int common_checks(eds_trk* h, int first, int count, bool needs_stride, int stride, int need) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (needs_stride && stride < max_points(h, first, count)) return fail(EDS_ERR_INVALID, "stride smaller than the largest point count");
    return check_idle_slots(h, first, count, need);
}

}  // namespace

int eds_kfp_check_transforms(int count, const double* T7, const double* K_dst) {
    for (int b = 0; b < count; ++b) {
        if (T7) {
            const double* q = T7 + 7 * (size_t)b + 3;
            if (!finite_all(T7 + 7 * (size_t)b, 7)) return fail(EDS_ERR_INVALID, "T7 is not finite");
            if (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] == 0.0) return fail(EDS_ERR_INVALID, "T7 holds a zero quaternion");
        }
        if (K_dst) {
            const double* K = K_dst + 4 * (size_t)b;
            if (!finite_all(K, 4) || K[0] == 0.0 || K[1] == 0.0) return fail(EDS_ERR_INVALID, "K_dst is not finite or has a zero focal length");
        }
    }
    return EDS_OK;
}

int eds_kfp_project_queue(eds_trk* h, int first, int cn, const double* T7, const double* K_dst, double dW, double dH, double* h_par,
                      const double* d_par, int* d_n, double* d_xy, double* d_idp, int* d_src) {
    for (int b = 0; b < cn; ++b) {
        const Slot& sl = h->slots[first + b];
        const double* p = T7 ? T7 + 7 * (size_t)b : sl.p;
        const double* qq = T7 ? T7 + 7 * (size_t)b + 3 : sl.q;
        double* P = h_par + (size_t)b * EDS_KFP_PAR;
        // R of the normalised quaternion (x, y, z, w), each entry as written, in fp64
        const double n = std::sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
        const double x = qq[0] / n, y = qq[1] / n, z = qq[2] / n, w = qq[3] / n;
        P[0] = 1.0 - 2.0 * (y * y + z * z); P[1] = 2.0 * (x * y - z * w);       P[2] = 2.0 * (x * z + y * w);
        P[3] = 2.0 * (x * y + z * w);       P[4] = 1.0 - 2.0 * (x * x + z * z); P[5] = 2.0 * (y * z - x * w);
        P[6] = 2.0 * (x * z - y * w);       P[7] = 2.0 * (y * z + x * w);       P[8] = 1.0 - 2.0 * (x * x + y * y);
        for (int j = 0; j < 3; ++j) P[9 + j] = p[j];
        for (int j = 0; j < 4; ++j) { P[12 + j] = sl.K[j]; P[16 + j] = K_dst ? K_dst[4 * (size_t)b + j] : sl.K[j]; }
        P[20] = dW; P[21] = dH; P[22] = sl.seeded ? 1.0 : 0.0; P[23] = 0.0;
    }
    hipLaunchKernelGGL(k_kfp_project, dim3(cn), dim3(EDS_KFP_PROJ_THREADS), 0, h->own.st, h->arrays(), first, d_par, h->depth.seeds, d_n,
                       d_xy, d_idp, d_src);
    EDS_HIP_TRY(hipGetLastError());
    return EDS_OK;
}

extern "C" {

int eds_kfp_abi_version(void) { return EDS_HIP_KFPOINTS_ABI_VERSION; }

int eds_kfp_refine_points(eds_trk* h, int first, int count, double event_diff, int patch_radius, int border_type, int border_value,
                          int erase, int stride, double* range, int32_t* kept_index, int* n_kept) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    const int r = patch_radius;
    if (r < 0 || r > EDS_KFP_MAX_RADIUS) return fail(EDS_ERR_INVALID, "patch_radius outside 0 .. 15");
    if (border_type != EDS_EPI_BORDER_CONSTANT && border_type != EDS_EPI_BORDER_REPLICATE && border_type != EDS_EPI_BORDER_REFLECT &&
        border_type != EDS_EPI_BORDER_REFLECT_101)
        return fail(EDS_ERR_INVALID, "unknown border type");
    if (border_value < 0 || border_value > 255) return fail(EDS_ERR_INVALID, "border_value outside 0 .. 255");
    if (erase != 0 && erase != 1) return fail(EDS_ERR_INVALID, "erase must be 0 or 1");
    if (!std::isfinite(event_diff)) return fail(EDS_ERR_INVALID, "event_diff is not finite");
    if ((rc = common_checks(h, first, count, range || kept_index, stride, EDS_NEED_KF | EDS_NEED_FRAME))) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = ensure_flags(h))) return rc;
    EdsKfpBuffers& k = h->kfp;
    const size_t Np = (size_t)h->Np;
    const int maxN = max_points(h, first, count);
    hipLaunchKernelGGL(k_kfp_range, dim3((maxN + EDS_KFP_WAVES - 1) / EDS_KFP_WAVES, count), dim3(64 * EDS_KFP_WAVES), 0, h->own.st, h->arrays(), first, r,
                       border_type, (float)border_value, event_diff, k.range, k.erase);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<double> vr;
    std::vector<int> n0(count);
    for (int b = 0; b < count; ++b) n0[b] = h->slots[first + b].N;
    if (range) { vr.resize(Np * count); EDS_HIP_TRY(hipMemcpyAsync(vr.data(), k.range + Np * first, Np * count * 8, hipMemcpyDeviceToHost, h->own.st)); }
    if ((rc = finish_erase(h, first, count, erase != 0, stride, kept_index, n_kept))) return rc;
    for (int b = 0; b < count; ++b) {
        if (erase) h->slots[first + b].num_points = h->slots[first + b].N;        // KeyFrame.cpp:1056
        if (range) std::memcpy(range + (size_t)b * stride, vr.data() + Np * b, (size_t)n0[b] * 8);
    }
    return EDS_OK;
}

int eds_kfp_clean_points(eds_trk* h, int first, int count, double w_norm_thr, int stride, int32_t* kept_index, int* n_kept) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (!std::isfinite(w_norm_thr)) return fail(EDS_ERR_INVALID, "w_norm_thr is not finite");
    if ((rc = common_checks(h, first, count, kept_index != nullptr, stride, EDS_NEED_KF))) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = ensure_flags(h))) return rc;
    hipLaunchKernelGGL(k_kfp_clean, dim3((max_points(h, first, count) + 255) / 256, count), dim3(256), 0, h->own.st, h->arrays(), first, w_norm_thr,
                       h->kfp.erase);
    EDS_HIP_TRY(hipGetLastError());
    return finish_erase(h, first, count, true, stride, kept_index, n_kept);
}

int eds_kfp_erase_points(eds_trk* h, int first, int count, int stride, const uint8_t* erase, int32_t* kept_index, int* n_kept) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (!erase) return fail(EDS_ERR_INVALID, "null erase flags");
    if ((rc = common_checks(h, first, count, true, stride, EDS_NEED_KF))) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = ensure_flags(h))) return rc;
    const size_t Np = (size_t)h->Np;
    std::vector<unsigned char> flags(Np * count, 0);
    for (int b = 0; b < count; ++b)
        for (int i = 0; i < h->slots[first + b].N; ++i) flags[Np * b + i] = erase[(size_t)b * stride + i] ? 1 : 0;
    EDS_HIP_TRY(hipMemcpyAsync(h->kfp.erase + Np * first, flags.data(), flags.size(), hipMemcpyHostToDevice, h->own.st));
    return finish_erase(h, first, count, true, stride, kept_index, n_kept);       // (waits for the stream before `flags` goes)
}

int eds_kfp_counts(eds_trk* h, int first, int count, int* num_points, int* current) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    for (int b = 0; b < count; ++b) {
        const Slot& s = h->slots[first + b];
        if (num_points) num_points[b] = s.num_points;
        if (current) current[b] = s.has_kf ? s.N : 0;
    }
    return EDS_OK;
}

int eds_kfp_project_depth_map(eds_trk* h, int first, int count, const double* T7, const double* K_dst, int dst_H, int dst_W, int stride,
                              double* depth_xy, double* depth_idp, int32_t* src_index, int* n_out) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if ((rc = eds_kfp_check_transforms(count, T7, K_dst))) return rc;
    if ((rc = common_checks(h, first, count, depth_xy || depth_idp || src_index, stride, EDS_NEED_KF))) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = ensure_project(h, std::min(count, EDS_KFP_BATCH)))) return rc;
    EdsKfpBuffers& k = h->kfp;
    const size_t Np = (size_t)h->Np;
    const double dW = (double)(dst_W > 0 ? dst_W : h->W), dH = (double)(dst_H > 0 ? dst_H : h->H);
    for (int c0 = 0; c0 < count; c0 += k.cap) {
        const int cn = std::min(k.cap, count - c0);
        if ((rc = eds_kfp_project_queue(h, first + c0, cn, T7 ? T7 + 7 * (size_t)c0 : nullptr, K_dst ? K_dst + 4 * (size_t)c0 : nullptr, dW, dH, k.h_par,
                                        k.d_par, k.d_n, k.d_xy, k.d_idp, k.d_src))) return rc;
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
        for (int b = 0; b < cn; ++b) {
            const int n = k.h_n[b];
            const size_t o = (size_t)(c0 + b) * stride;
            if (depth_xy && n > 0) std::memcpy(depth_xy + 2 * o, k.h_xy + 2 * Np * b, (size_t)n * 16);
            if (depth_idp && n > 0) std::memcpy(depth_idp + o, k.h_idp + Np * b, (size_t)n * 8);
            if (src_index && n > 0) std::memcpy(src_index + o, k.h_src + Np * b, (size_t)n * 4);
            if (n_out) n_out[c0 + b] = n;
        }
    }
    return EDS_OK;
}

}  // extern "C"
