// The KLT point trackers of EDS on the device (include/eds_hip_klt.h): Tracker::trackPoints / trackPointsPyr (reference
// src/tracking/Tracker.cpp:378-488) for the points of a tracker slot.
//
//   k_update_points  getCoord(true) (eds_points.hip) with its coordinates and kept indices in HBM, the re-projection tracks in the
//                    tracks plane and the flow plane compacted behind the kept indices
//   k_klt_bin        one workgroup per alignment: the points binned by splat row.  One key (eds_splat.hpp) per point; a counting
//                    sort by y0, then a rank sort inside each row, so that each row's keys ascend in (x0, i).  [B][Np] keys and
//                    [B][H + 2] row starts: no per-pixel scratch
//   k_klt_window     one wavefront per point: its window's reflect-101 positions (splitImageInPatches, Utils.cpp:608-633), the splat
//                    values of the box they and the blur reach and the 3 x 3 Gaussian blur (both eds_splat.hpp), pyrDown levels
//                    (pyramidPatches, Utils.cpp:662-673), kltTracker's five sums (Utils.cpp:735-759) as shuffle reductions and
//                    the 2 x 2 solve in Eigen's closed form; then flow / tracks
//
// fp64 throughout, and this translation unit is compiled WITHOUT fp contraction (Makefile).  No float atomics: every sum has a
// fixed order, so a batch equals its singles bit for bit and runs repeat exactly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/eds_hip_klt.h"
#include "eds_capi_internal.hpp"
#include "eds_device.hpp"
#include "eds_splat.hpp"

using namespace edscapi;
using namespace edsd;
using namespace edssplat;

#define EDS_KLT_BIN_THREADS 1024
#define EDS_KLT_MAX_RADIUS 31
#define EDS_KLT_MAX_LEVEL 5
#define EDS_KLT_HDR_INTS 272        // window kernel LDS header: reflected columns [64], rows [64], row key ranges [72] x 2

namespace {

// getCoord(true) keeps 0 <= x <= cols, 0 <= y <= rows (and lets NaN through): only such points are binned
__device__ __forceinline__ bool binned(double x, double y, int W, int H) { return x >= 0.0 && x <= (double)W && y >= 0.0 && y <= (double)H; }
// bias 1 (the epiline model, whose keyframe pixels no getCoord has erased): every point whose footprint touches the image,
// -1 < x < cols, -1 < y < rows, keyed (y0 + 1, x0 + 1) so that the row and column left of the frame fit the unsigned key
__device__ __forceinline__ bool binned(double x, double y, int W, int H, int bias) {
    return bias ? (x > -1.0 && x < (double)W && y > -1.0 && y < (double)H) : binned(x, y, W, H);
}

__global__ __launch_bounds__(EDS_KLT_BIN_THREADS) void k_klt_bin(EdsArrays A, int first, const double* __restrict__ coord,
                                                                uint64_t* __restrict__ keys_tmp, uint64_t* __restrict__ keys,
                                                                int* __restrict__ row_start, int bias) {
    extern __shared__ int s_bin[];          // [H + 2] row starts, [H + 2] cursors
    const int slot = first + blockIdx.x, tid = threadIdx.x, H = A.H, W = A.W;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const size_t base = (size_t)slot * A.Np;
    coord += 2 * base; keys_tmp += base; keys += base; row_start += (size_t)slot * (H + 2);
    int* s_cur = s_bin + (H + 2);
    for (int y = tid; y < H + 2; y += EDS_KLT_BIN_THREADS) s_bin[y] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += EDS_KLT_BIN_THREADS) {
        const double x = coord[2 * i], y = coord[2 * i + 1];
        if (binned(x, y, W, H, bias)) atomicAdd(&s_bin[(int)floor(y) + bias], 1);         // (integer counts: the same in any order)
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int y = 0; y <= H; ++y) { const int c = s_bin[y]; s_bin[y] = run; s_cur[y] = run; run += c; }
        s_bin[H + 1] = run;
    }
    __syncthreads();
    for (int y = tid; y < H + 2; y += EDS_KLT_BIN_THREADS) row_start[y] = s_bin[y];
    for (int i = tid; i < N; i += EDS_KLT_BIN_THREADS) {
        const double x = coord[2 * i], y = coord[2 * i + 1];
        if (!binned(x, y, W, H, bias)) continue;
        const int y0 = (int)floor(y) + bias, x0 = (int)floor(x) + bias;
        const int pos = atomicAdd(&s_cur[y0], 1);                             // arrival order; the rank sort below fixes it
        keys_tmp[pos] = splat_key(y0, x0, i);
    }
    __threadfence_block();
    __syncthreads();
    const int nb = s_bin[H + 1];
    for (int p = tid; p < nb; p += EDS_KLT_BIN_THREADS) {
        const uint64_t k = keys_tmp[p];
        const int y0 = key_y0(k);
        const int lo = s_bin[y0], hi = s_bin[y0 + 1];
        int rank = 0;
        for (int q = lo; q < hi; ++q) rank += keys_tmp[q] < k ? 1 : 0;
        keys[lo + rank] = k;
    }
}

// kltTracker's return value -M^-1 b with Eigen's 2 x 2 inverse (invdet = 1 / (m00 m11 - m10 m01), cofactors times invdet)
__device__ __forceinline__ void klt_solve(double sxx, double syy, double sxy, double sxt, double syt, double& f0, double& f1) {
    const double det = sxx * syy - sxy * sxy;
    const double invdet = 1.0 / det;
    const double i00 = syy * invdet, i10 = -sxy * invdet, i01 = -sxy * invdet, i11 = sxx * invdet;
    f0 = -i00 * sxt + -i01 * syt;
    f1 = -i10 * sxt + -i11 * syt;
}

// One wavefront per point i = blockIdx.x of alignment blockIdx.y.  LDS: the header, the splat box of both gradients (fp64) and, for
// the pyramid variant, levels 1.. of the three windows (fp64, two buffers taken in turn).
template <bool PYR>
__global__ __launch_bounds__(64) void k_klt_window(EdsArrays A, int first, int r, int L, double k0, double k1, double k2,
                                                   const double* __restrict__ coord, const uint64_t* __restrict__ keys,
                                                   const int* __restrict__ row_start, double* __restrict__ tracks, double* __restrict__ flow) {
    extern __shared__ double s_lds[];
    const int i = blockIdx.x, slot = first + blockIdx.y, lane = threadIdx.x;
    const double* pbk = A.pose + (size_t)slot * EDS_POSE_STRIDE;
    const int N = (int)pbk[EDS_PB_N];
    if (i >= N) return;
    const int H = A.H, W = A.W, S = 2 * r + 1;
    const size_t base = (size_t)slot * A.Np, plane = (size_t)A.B * A.Np;
    const double* __restrict__ C = coord + 2 * base;
    const uint64_t* __restrict__ K = keys + base;
    const int* __restrict__ RS = row_start + (size_t)slot * (H + 2);
    const double x = C[2 * i], y = C[2 * i + 1];
    double f0 = __builtin_nan(""), f1 = __builtin_nan("");
    if (binned(x, y, W, H)) {
        int* s_ox = reinterpret_cast<int*>(s_lds);
        int* s_oy = s_ox + 64;
        int* s_rlo = s_oy + 64;
        int* s_rhi = s_rlo + 72;
        double* s_box = s_lds + EDS_KLT_HDR_INTS / 2;
        // the window on the image padded by r (copyMakeBorder, reflect-101) starts at the TRUNCATED coordinates (cv::Rect of a
        // Point2d): padded column tx + k is image column reflect101(tx - r + k)
        const int tx = (int)x, ty = (int)y;
        const int oxk = lane < S ? reflect101(tx - r + lane, W) : 0, oyk = lane < S ? reflect101(ty - r + lane, H) : 0;
        if (lane < S) { s_ox[lane] = oxk; s_oy[lane] = oyk; }
        int mnx = lane < S ? oxk : INT_MAX, mxx = lane < S ? oxk : INT_MIN, mny = lane < S ? oyk : INT_MAX, mxy = lane < S ? oyk : INT_MIN;
        for (int off = 1; off < 64; off <<= 1) {
            mnx = min(mnx, __shfl_xor(mnx, off, 64)); mxx = max(mxx, __shfl_xor(mxx, off, 64));
            mny = min(mny, __shfl_xor(mny, off, 64)); mxy = max(mxy, __shfl_xor(mxy, off, 64));
        }
        // the splat pixels the blurred window reads: its positions +- 1, inside the image
        const int bx0 = max(0, mnx - 1), bx1 = min(W - 1, mxx + 1), by0 = max(0, mny - 1), by1 = min(H - 1, mxy + 1);
        const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
        // key ranges of the splat rows y0 = by0 - 1 .. by1 restricted to x0 = bx0 - 1 .. bx1: the footprints that reach the box
        for (int j = lane; j <= bh; j += 64) {
            const int yy = by0 - 1 + j;
            int lo = 0, hi = 0;
            if (yy >= 0) {
                lo = RS[yy]; hi = RS[yy + 1];
                lo = lower_x(K, lo, hi, bx0 - 1);
                hi = lower_x(K, lo, hi, bx1 + 1);
            }
            s_rlo[j] = lo; s_rhi[j] = hi;
        }
        __syncthreads();
        // drawValuesPoints' bilinear splat of both gradients at each box pixel (py, px), py = by0 + jy: the runs of rows py - 1 (range
        // index jy) and py (jy + 1), each scanned forward from the row's pre-bisected start
        const int nbox = bw * bh;
        const float* const G[2] = {A.gx + base, A.gy + base};
        for (int p = lane; p < nbox; p += 64) {
            const int jy = p / bw, px = bx0 + p - jy * bw;
            int g[4][2];
            for (int h2 = 0; h2 < 2; ++h2) {
                const int hi = s_rhi[jy + h2];
                int q = s_rlo[jy + h2];
                while (q < hi && key_x0(K[q]) < px - 1) ++q;
                splat_runs(K, q, hi, px - 1, g + 2 * h2);
            }
            double s[2];
            splat_merge(K, g, C, G, s);
            s_box[p] = s[0];
            s_box[nbox + p] = s[1];
        }
        __syncthreads();
        const FrameView fv = make_frame_view(A.frame, (int)pbk[EDS_PB_FRAME], H, W, A.Hp, A.Wp, A.tiled);
        // level-0 window value of channel ch (0: blurred grad_x, 1: blurred grad_y, 2: event frame) at window row kr, column kc
        auto level0 = [&](int ch, int kr, int kc) -> double {
            const int oy = s_oy[kr], ox = s_ox[kc];
            if (ch == 2) return (double)fv.base[frame_index(fv, oy, ox)];
            return blur3_at(s_box + ch * nbox, bw, bx0, by0, ox, oy, W, H, k0, k1, k2);
        };
        double kl[EDS_KLT_MAX_LEVEL][2];
        if (PYR && L > 1) {
            // pyrDown (5 x 5 [1 4 6 4 1]^2 / 256, reflect-101 inside the patch): horizontally c 6 + (l1 + r1) 4 + l2 + r2, then the same
            // vertically, times 1/256.  Level 1 straight from the level-0 values; level j (>= 1) lives in lv[(j - 1) & 1].
            const int s1 = S / 2;
            double* lv[2] = {s_box + 2 * nbox, s_box + 2 * nbox + 3 * s1 * s1};
            for (int j = 1; j < L; ++j) {
                const int sp = S >> (j - 1), sn = S >> j;
                const double* src = j >= 2 ? lv[(j - 2) & 1] : nullptr;
                double* dst = lv[(j - 1) & 1];
                const int splane = sp * sp, dplane = sn * sn;
                for (int p = lane; p < 3 * dplane; p += 64) {
                    const int ch = p / dplane, q = p - ch * dplane, yy = q / sn, xx = q - yy * sn;
                    double rows[5];
                    for (int t = 0; t < 5; ++t) {
                        const int ry = reflect101(2 * yy + t - 2, sp);
                        double v[5];
                        for (int u = 0; u < 5; ++u) {
                            const int cx = reflect101(2 * xx + u - 2, sp);
                            v[u] = j == 1 ? level0(ch, ry, cx) : src[ch * splane + ry * sp + cx];
                        }
                        rows[t] = v[2] * 6.0 + (v[1] + v[3]) * 4.0 + v[0] + v[4];
                    }
                    dst[ch * dplane + q] = (rows[2] * 6.0 + (rows[1] + rows[3]) * 4.0 + rows[0] + rows[4]) * 0.00390625;
                }
                __syncthreads();
                double sxx = 0.0, syy = 0.0, sxy = 0.0, sxt = 0.0, syt = 0.0;
                for (int q = lane; q < dplane; q += 64) {
                    const double ix = dst[q], iy = dst[dplane + q], it = dst[2 * dplane + q];
                    sxx += ix * ix; syy += iy * iy; sxy += ix * iy; sxt += ix * it; syt += iy * it;
                }
                klt_solve(wave_sum(sxx), wave_sum(syy), wave_sum(sxy), wave_sum(sxt), wave_sum(syt), kl[j][0], kl[j][1]);
            }
        }
        {   // level 0 (the only one of trackPoints): kltTracker on the full windows
            double sxx = 0.0, syy = 0.0, sxy = 0.0, sxt = 0.0, syt = 0.0;
            for (int p = lane; p < S * S; p += 64) {
                const int kr = p / S, kc = p - kr * S;
                const double ix = level0(0, kr, kc), iy = level0(1, kr, kc), it = level0(2, kr, kc);
                sxx += ix * ix; syy += iy * iy; sxy += ix * iy; sxt += ix * it; syt += iy * it;
            }
            klt_solve(wave_sum(sxx), wave_sum(syy), wave_sum(sxy), wave_sum(sxt), wave_sum(syt), kl[0][0], kl[0][1]);
        }
        if (PYR) {
            // f += (1 / scale) * klt_j / scale, coarsest first, no warping between levels (Tracker.cpp:466-473)
            f0 = 0.0; f1 = 0.0;
            for (int j = L - 1; j >= 0; --j) {
                const double scale = (double)(1 << j);
                f0 += (1.0 / scale) * kl[j][0] / scale;
                f1 += (1.0 / scale) * kl[j][1] / scale;
            }
        } else {
            f0 = kl[0][0]; f1 = kl[0][1];
        }
    }
    if (lane == 0) {
        const size_t o = base + i;
        if (PYR) { flow[o] += f0; flow[plane + o] += f1; }          // kf->flow[i] += f (Tracker.cpp:479)
        else { flow[o] = f0; flow[plane + o] = f1; }                // kf->flow[idx] = f (:413)
        tracks[o] += f0; tracks[plane + o] += f1;                   // kf->tracks[i] += f (:417, :481)
    }
}

int ensure(eds_trk* h) {
    EdsKltBuffers& k = h->klt;
    if (k.tracks) return EDS_OK;
    const size_t B = (size_t)h->B, Np = (size_t)h->Np, H = (size_t)h->H;
    if (!h->own.alloc({{(void**)&k.tracks, 2 * B * Np * 8}, {(void**)&k.flow, 2 * B * Np * 8}, {(void**)&k.coord, 2 * B * Np * 8},
                       {(void**)&k.kept, B * Np * 4}, {(void**)&k.keys_tmp, B * Np * 8}, {(void**)&k.keys, B * Np * 8},
                       {(void**)&k.row_start, B * (H + 2) * 4}}))
        return fail(EDS_ERR_HIP, "allocation of the KLT buffers failed");
    // every KeyFrame::create zeroes flow (KeyFrame.cpp:447-448); tracks are zero until getCoord writes them
    EDS_HIP_TRY(hipMemsetAsync(k.tracks, 0, 2 * B * Np * 8, h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(k.flow, 0, 2 * B * Np * 8, h->own.st));
    return EDS_OK;
}

size_t window_lds(const eds_trk* h, int r, int L, bool pyr) {
    const size_t bw = (size_t)std::min(h->W, 2 * r + 3), bh = (size_t)std::min(h->H, 2 * r + 3);
    size_t bytes = EDS_KLT_HDR_INTS * 4 + 2 * bw * bh * 8;
    if (pyr && L > 1) {
        const size_t s1 = (size_t)(2 * r + 1) / 2, s2 = (size_t)(2 * r + 1) / 4;
        bytes += 3 * (s1 * s1 + s2 * s2) * 8;
    }
    return bytes;
}

int run(eds_trk* h, int first, int count, int r, int L, bool pyr, int stride, double* coord_xy, double* tracks_xy, double* flow_xy,
        int32_t* kept_index, int* n_kept) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (pyr ? (L < 1 || L > EDS_KLT_MAX_LEVEL) : (r < 0 || r > EDS_KLT_MAX_RADIUS))
        return fail(EDS_ERR_INVALID, pyr ? "num_level outside 1 .. 5" : "patch_radius outside 0 .. 31");
    if ((coord_xy || tracks_xy || flow_xy || kept_index) && stride < max_points(h, first, count))
        return fail(EDS_ERR_INVALID, "stride smaller than the largest point count");
    if ((rc = check_idle_slots(h, first, count, EDS_NEED_KF | EDS_NEED_FRAME))) return rc;
    const size_t bin_lds = 2 * ((size_t)h->H + 2) * 4, win_lds = window_lds(h, r, L, pyr);
    size_t max_lds = 0;
    if ((rc = workgroup_lds_limit(h, &max_lds))) return rc;
    if (!row_bins_fit(h, max_lds) || win_lds > max_lds)
        return fail(EDS_ERR_NOT_USABLE, "the KLT windows or the row bins of this frame size do not fit the workgroup's LDS");
    if ((rc = ensure(h))) return rc;
    EdsKltBuffers& kb = h->klt;
    // 1. getCoord(true): coordinates and kept indices into HBM, tracks into the plane, seeds and flow compacted
    const EdsPointsDev dev = {kb.coord, kb.kept};
    if ((rc = update_points_range(h, first, count, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &dev))) return rc;
    const int maxN = max_points(h, first, count);
    // 2. bins, 3. windows
    hipLaunchKernelGGL(k_klt_bin, dim3(count), dim3(EDS_KLT_BIN_THREADS), bin_lds, h->own.st, h->arrays(), first, kb.coord, kb.keys_tmp, kb.keys,
                       kb.row_start, 0);
    EDS_HIP_TRY(hipGetLastError());
    double k0, k1;
    gauss3_sigma_half(k0, k1);
    if (maxN > 0) {
        if (pyr)
            hipLaunchKernelGGL(k_klt_window<true>, dim3(maxN, count), dim3(64), win_lds, h->own.st, h->arrays(), first, r, L, k0, k1, k0, kb.coord,
                               kb.keys, kb.row_start, kb.tracks, kb.flow);
        else
            hipLaunchKernelGGL(k_klt_window<false>, dim3(maxN, count), dim3(64), win_lds, h->own.st, h->arrays(), first, r, L, k0, k1, k0, kb.coord,
                               kb.keys, kb.row_start, kb.tracks, kb.flow);
        EDS_HIP_TRY(hipGetLastError());
    }
    // 4. what the caller asked for
    const size_t Np = (size_t)h->Np, n = (size_t)count * Np;
    std::vector<double> va;
    std::vector<int32_t> vk;
    if (coord_xy) { va.resize(2 * n); EDS_HIP_TRY(hipMemcpyAsync(va.data(), kb.coord + 2 * Np * first, 2 * n * 8, hipMemcpyDeviceToHost, h->own.st)); }
    if (kept_index) { vk.resize(n); EDS_HIP_TRY(hipMemcpyAsync(vk.data(), kb.kept + Np * first, n * 4, hipMemcpyDeviceToHost, h->own.st)); }
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    for (int b = 0; b < count; ++b) {
        const int nk = h->slots[first + b].N;
        const size_t o = (size_t)b * stride;
        if (n_kept) n_kept[b] = nk;
        if (coord_xy && nk > 0) std::memcpy(coord_xy + 2 * o, va.data() + 2 * Np * b, (size_t)nk * 16);
        if (kept_index && nk > 0) std::memcpy(kept_index + o, vk.data() + Np * b, (size_t)nk * 4);
    }
    if (tracks_xy && (rc = read_xy_planes(h, kb.tracks, first, count, stride, tracks_xy))) return rc;
    if (flow_xy && (rc = read_xy_planes(h, kb.flow, first, count, stride, flow_xy))) return rc;
    return EDS_OK;
}

}  // namespace

int eds_klt_bin_launch(eds_trk* h, int first, int count, const double* coord, uint64_t* keys_tmp, uint64_t* keys, int* row_start, int bias) {
    hipLaunchKernelGGL(k_klt_bin, dim3(count), dim3(EDS_KLT_BIN_THREADS), 2 * ((size_t)h->H + 2) * 4, h->own.st, h->arrays(), first, coord, keys_tmp,
                       keys, row_start, bias);
    return hipGetLastError() == hipSuccess ? EDS_OK : fail(EDS_ERR_HIP, "launch of k_klt_bin failed");
}

void eds_klt_reset_slot(eds_trk* h, int slot) {
    if (!h->klt.tracks) return;
    const size_t Np = (size_t)h->Np, plane = (size_t)h->B * Np, o = (size_t)slot * Np;
    for (double* p : {h->klt.tracks, h->klt.flow}) {
        hipMemsetAsync(p + o, 0, Np * 8, h->own.st);
        hipMemsetAsync(p + plane + o, 0, Np * 8, h->own.st);
    }
}

extern "C" {

int eds_klt_abi_version(void) { return EDS_HIP_KLT_ABI_VERSION; }

int eds_klt_track_points(eds_trk* h, int first, int count, int patch_radius, int stride, double* coord_xy, double* tracks_xy,
                         double* flow_xy, int32_t* kept_index, int* n_kept) {
    return run(h, first, count, patch_radius, 1, false, stride, coord_xy, tracks_xy, flow_xy, kept_index, n_kept);
}

int eds_klt_track_points_pyr(eds_trk* h, int first, int count, int num_level, int stride, double* coord_xy, double* tracks_xy,
                             double* flow_xy, int32_t* kept_index, int* n_kept) {
    // uint16_t patch_radius = 3 * 2^(L-1) + L; patch_radius /= 2 (Tracker.cpp:440-441)
    const int r = (num_level >= 1 && num_level <= EDS_KLT_MAX_LEVEL) ? (3 * (1 << (num_level - 1)) + num_level) / 2 : 0;
    return run(h, first, count, r, num_level, true, stride, coord_xy, tracks_xy, flow_xy, kept_index, n_kept);
}

int eds_klt_get(eds_trk* h, int slot, double* tracks_xy, double* flow_xy) {
    int rc = check_slot(h, slot);
    if (rc) return rc;
    if (!tracks_xy && !flow_xy) return fail(EDS_ERR_INVALID, "null output");
    if ((rc = check_idle_slots(h, slot, 1, EDS_NEED_KF))) return rc;
    if (!h->klt.tracks) return fail(EDS_ERR_STATE, "no device tracks: eds_klt_track_points has not run on this handle");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const int N = h->slots[slot].N;
    if (tracks_xy && (rc = read_xy_planes(h, h->klt.tracks, slot, 1, N, tracks_xy))) return rc;
    if (flow_xy && (rc = read_xy_planes(h, h->klt.flow, slot, 1, N, flow_xy))) return rc;
    return EDS_OK;
}

}  // extern "C"
