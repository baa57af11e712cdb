// The epiline tracker of EDS on the device (include/eds_hip_epiline.h): Tracker::trackPointsAlongEpiline (reference
// src/tracking/Tracker.cpp:490-553) for the points of a tracker slot.
//
//   k_epi_values     one workgroup per alignment: getSparseModel (KeyFrame.cpp:1358-1403) — the keyframe pixel the slot holds, the
//                    flow compute_flow(norm_coord, v, w, mu) (Utils.hpp:165-173), m = -(g . f), then m / sqrt(1e-3 + sum m^2) with
//                    the sum in point order
//   k_klt_bin        (eds_klt.hip) the keyframe pixels binned by splat row: keys (y0 + 1, x0 + 1, i), no per-pixel scratch.  The bias
//                    of one keeps the points with x or y in (-1, 0): their x1 / y1 corners land on column / row 0 with the
//                    reference's weights (Utils.cpp:164-178); no getCoord has erased them, as it has for the KLT
//   k_epi_model      the splat of those keys and its 3 x 3 Gaussian blur (both eds_splat.hpp) per 32 x 8 tile: the model image
//                    [B][H][W] in fp64
//   k_epi_templates  one wavefront per point: splitImageInPatches (Utils.cpp:608-633) at the TRUNCATED keyframe pixel, the patch in
//                    fp32, S = sum T^2 exactly in fp64, and the non-zero taps compacted in row-major order as (LDS offset, value)
//   k_epi_pad        copyMakeBorder(event_frame, r, border) in fp32 (Tracker.cpp:505-506)
//   k_epi_rowsq / k_epi_energy   E = the window sums of P^2 in fp64 (separable), kept as fp32 (E, sqrt E) per position
//   k_epi_match      the hot path.  One workgroup per (64 x 32 tile of positions, 32 templates, alignment): the tile's padded image
//                    in LDS, per template C = sum_taps P T over its NON-ZERO taps in fp32 (8 positions per lane), the two normed scores
//                    and their arg-extrema fused behind it; one 64-bit atomicMin per wavefront and method on a (orderable fp32 score,
//                    row-major index) key.  No (position, template) value is ever stored, no float atomics.
//   k_epi_finish     per point: the locations and scores from the keys, the cull |‖p_ssd‖ - ‖p_ncc‖| > 5 in fp64
//   then getCoord's compaction (k_update_points, eds_points.hip) erases the culled points by flag, with the seeds and the KLT's
//   tracks and flow; k_epi_gather writes the kept points' p_ssd into the ef plane.
//
// The model image and templates are fp64 without FMA contraction: this translation unit is compiled with -ffp-contract=off (Makefile);
// the correlation's fp32 multiply-adds are explicit fmaf.  Every sum has a fixed order and the cross-workgroup combine is an integer
// min, so a batch equals its singles bit for bit and runs repeat exactly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/eds_hip_epiline.h"
#include "../../include/eds_hip_depth.h"
#include "eds_capi_internal.hpp"
#include "eds_depth.hpp"
#include "eds_device.hpp"
#include "eds_splat.hpp"

using namespace edscapi;
using namespace edsd;
using namespace edssplat;

#define EDS_EPI_MAX_RADIUS 15
#define EDS_EPI_PAR 16              // per slot: fx fy cx cy, v[6], seeded
#define EDS_EPI_VAL_THREADS 1024
#define EDS_EPI_MODEL_TW 32         // k_epi_model tile
#define EDS_EPI_MODEL_TH 8
#define EDS_EPI_TW 64               // k_epi_match tile: one column per lane ...
#define EDS_EPI_ROWS 8              // ... EDS_EPI_ROWS rows per lane ...
#define EDS_EPI_TH (4 * EDS_EPI_ROWS)   // ... four wavefronts
#define EDS_EPI_GROUP 32            // templates per workgroup
#define EDS_EPI_CHUNK 16            // alignments per pass of the per-radius work buffers

namespace {

// fp32 score -> unsigned key ascending with the score; -0 and +0 map to the same key
__device__ __forceinline__ unsigned ord_key(float s) {
    const unsigned u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_val(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(EDS_EPI_VAL_THREADS) void k_epi_values(EdsArrays A, int first, const double* __restrict__ par,
                                                                    const double* __restrict__ seeds_mu, double* __restrict__ kpix,
                                                                    double* __restrict__ mval) {
    __shared__ double s_sq[EDS_EPI_VAL_THREADS];
    __shared__ double s_norm;
    const int slot = first + blockIdx.x, tid = threadIdx.x;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const double* P = par + (size_t)slot * EDS_EPI_PAR;
    const double fx = P[0], fy = P[1], cx = P[2], cy = P[3];
    const double v0 = P[4], v1 = P[5], v2 = P[6], w0 = P[7], w1 = P[8], w2 = P[9];
    const bool seeded = P[10] != 0.0;
    const size_t base = (size_t)slot * A.Np;
    for (int i = tid; i < N; i += EDS_EPI_VAL_THREADS) {
        const size_t o = base + i;
        const int c = A.cell0[o];
        const double u = (double)(short)(c & 0xffff) + (double)A.f0x[o], v = (double)(c >> 16) + (double)A.f0y[o];
        kpix[2 * o] = u; kpix[2 * o + 1] = v;
        const double xp = (u - cx) / fx, yp = (v - cy) / fy;                  // KeyFrame.cpp:1373-1374
        const double idp = seeded ? seeds_mu[o] : (double)A.rho[o];           // mu(inv_depth)
        // compute_flow, left to right as written (Utils.hpp:165-173); std::pow(x, 2) is x * x correctly rounded
        const double f0 = (-idp * v0) + (xp * idp * v2) + (xp * yp * w0) - (1.0 + xp * xp) * w1 + (yp * w2);
        const double f1 = (-idp * v1) + (yp * idp * v2) + (1.0 + yp * yp) * w0 - (xp * yp * w1) - (xp * w2);
        mval[o] = -((double)A.gx[o] * f0 + (double)A.gy[o] * f1);
    }
    // model_norm_sq = 1e-3 + sum m^2 in point order (:1386-1394): squares staged per chunk, one lane adds them in order
    double acc = 1e-03;
    for (int c0 = 0; c0 < N; c0 += EDS_EPI_VAL_THREADS) {
        const int i = c0 + tid;
        if (i < N) { const double m = mval[base + i]; s_sq[tid] = m * m; }      // (this lane wrote mval[base + i] above)
        __syncthreads();
        if (tid == 0) {
            const int n = min(EDS_EPI_VAL_THREADS, N - c0);
            for (int j = 0; j < n; ++j) acc += s_sq[j];
        }
        __syncthreads();
    }
    if (tid == 0) s_norm = sqrt(acc);
    __syncthreads();
    const double norm = s_norm;
    for (int i = tid; i < N; i += EDS_EPI_VAL_THREADS) mval[base + i] = mval[base + i] / norm;
}

// drawValuesPoints + GaussianBlur 3 x 3 of one 32 x 8 tile of alignment blockIdx.y
__global__ __launch_bounds__(256) void k_epi_model(EdsArrays A, int first, double k0, double k1, double k2, const double* __restrict__ kpix,
                                                   const double* __restrict__ mval, const uint64_t* __restrict__ keys,
                                                   const int* __restrict__ row_start, double* __restrict__ model) {
    __shared__ double s_box[(EDS_EPI_MODEL_TW + 2) * (EDS_EPI_MODEL_TH + 2)];
    const int slot = first + blockIdx.y, tid = threadIdx.x, H = A.H, W = A.W;
    const int ntx = (W + EDS_EPI_MODEL_TW - 1) / EDS_EPI_MODEL_TW;
    const int tx0 = (blockIdx.x % ntx) * EDS_EPI_MODEL_TW, ty0 = (blockIdx.x / ntx) * EDS_EPI_MODEL_TH;
    const size_t base = (size_t)slot * A.Np;
    const double* __restrict__ Cd = kpix + 2 * base;
    const double* const V[1] = {mval + base};
    const uint64_t* __restrict__ K = keys + base;
    const int* __restrict__ RS = row_start + (size_t)slot * (H + 2);
    // the splat pixels the blurred tile reads: its pixels +- 1, inside the image (reflect-101 of -1 / W lands inside this box)
    const int bx0 = max(0, tx0 - 1), bx1 = min(W - 1, tx0 + EDS_EPI_MODEL_TW), by0 = max(0, ty0 - 1), by1 = min(H - 1, ty0 + EDS_EPI_MODEL_TH);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    for (int p = tid; p < bw * bh; p += 256) {
        const int jy = p / bw, py = by0 + jy, px = bx0 + p - jy * bw;
        // The keys and row starts carry a bias of one: y0 = -1 and x0 = -1 are row 0 and key column 0, so the runs of rows
        // y0 = py - 1, py at x0 = px - 1, px are those of key rows py, py + 1 at key columns px, px + 1
        int g[4][2];
        for (int h2 = 0; h2 < 2; ++h2) {
            const int hi = RS[py + h2 + 1];
            splat_runs(K, lower_x(K, RS[py + h2], hi, px), hi, px, g + 2 * h2);
        }
        double s[1];
        splat_merge(K, g, Cd, V, s);
        s_box[p] = s[0];
    }
    __syncthreads();
    const int ly = tid / EDS_EPI_MODEL_TW, lx = tid - ly * EDS_EPI_MODEL_TW;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) return;
    model[(size_t)slot * H * W + (size_t)y * W + x] = blur3_at(s_box, bw, bx0, by0, x, y, W, H, k0, k1, k2);
}

// one wavefront per point i = blockIdx.x of chunk alignment blockIdx.y (slot first + blockIdx.y)
__global__ __launch_bounds__(64) void k_epi_templates(EdsArrays A, int first, int r, int border, double bval, int pitch,
                                                      const double* __restrict__ kpix, const double* __restrict__ model,
                                                      int2* __restrict__ taps, float4* __restrict__ tmeta) {
    const int i = blockIdx.x, b = blockIdx.y, slot = first + b, lane = threadIdx.x, H = A.H, W = A.W;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (i >= N) return;
    const int S = 2 * r + 1, K = S * S;
    const size_t o = (size_t)slot * A.Np + i, t = (size_t)b * A.Np + i;
    // cv::Rect of a Point2d: the coordinates TRUNCATED.  The slot's pixel is cell + fp32 fraction, so a pixel that fx ((u - cx) / fx) + cx
    // put 1e-13 below an integer u holds the fraction 1.0f and comes back as u exactly
    const int tx = (int)kpix[2 * o], ty = (int)kpix[2 * o + 1];
    const double* __restrict__ M = model + (size_t)slot * H * W;
    int2* __restrict__ T = taps + t * K;
    int cnt = 0;
    double ss = 0.0;
    for (int j0 = 0; j0 < K; j0 += 64) {
        const int j = j0 + lane;
        float v = 0.0f;
        int off = 0;
        if (j < K) {
            const int ky = j / S, kx = j - ky * S;
            const int my = ty - r + ky, mx = tx - r + kx;           // the padded model's (ty + ky, tx + kx)
            double mv;
            if (border == EDS_EPI_BORDER_CONSTANT && ((unsigned)my >= (unsigned)H || (unsigned)mx >= (unsigned)W)) mv = bval;
            else mv = M[(size_t)border_map(my, H, border) * W + border_map(mx, W, border)];
            v = (float)mv;                                           // convertTo(CV_32FC1) (Tracker.cpp:524)
            off = ky * pitch + kx;
            ss += (double)v * (double)v;
        }
        const bool nz = j < K && v != 0.0f;
        const unsigned long long m = __ballot(nz);
        if (nz) {
            const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            T[pos] = make_int2(off, __float_as_int(v));
        }
        cnt += __popcll(m);
    }
    ss = wave_sum(ss);
    if (lane == 0) tmeta[t] = make_float4(__int_as_float(cnt), (float)ss, (float)sqrt(ss), 0.0f);
}

// copyMakeBorder(event_frame, r, border, bval) in fp32, [chunk][(H + 2r) (W + 2r)]
__global__ __launch_bounds__(256) void k_epi_pad(EdsArrays A, int first, int r, int border, float bval, float* __restrict__ pad) {
    const int b = blockIdx.y, slot = first + b, H = A.H, W = A.W, Wp2 = W + 2 * r, Hp2 = H + 2 * r;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Hp2 * Wp2) return;
    const int py = q / Wp2, px = q - py * Wp2, iy = py - r, ix = px - r;
    float v;
    if (border == EDS_EPI_BORDER_CONSTANT && ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W)) v = bval;
    else {
        const FrameView fv = make_frame_view(A.frame, (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_FRAME], H, W, A.Hp, A.Wp, A.tiled);
        v = fv.base[frame_index(fv, border_map(iy, H, border), border_map(ix, W, border))];
    }
    pad[(size_t)b * Hp2 * Wp2 + q] = v;
}

// row sums of P^2 over 2r + 1 columns, [chunk][(H + 2r) W] fp64
__global__ __launch_bounds__(256) void k_epi_rowsq(int H, int W, int r, const float* __restrict__ pad, double* __restrict__ rowsq) {
    const int b = blockIdx.y, Wp2 = W + 2 * r, Hp2 = H + 2 * r;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Hp2 * W) return;
    const int py = q / W, x = q - py * W;
    const float* P = pad + (size_t)b * Hp2 * Wp2 + (size_t)py * Wp2 + x;
    double s = 0.0;
    for (int k = 0; k <= 2 * r; ++k) s += (double)P[k] * (double)P[k];
    rowsq[(size_t)b * Hp2 * W + q] = s;
}

// E of every position = the column sums of the row sums; kept as fp32 (E, sqrt E)
__global__ __launch_bounds__(256) void k_epi_energy(int H, int W, int r, const double* __restrict__ rowsq, float2* __restrict__ energy) {
    const int b = blockIdx.y, Hp2 = H + 2 * r;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= H * W) return;
    const int y = q / W, x = q - y * W;
    const double* R = rowsq + (size_t)b * Hp2 * W + (size_t)y * W + x;
    double e = 0.0;
    for (int k = 0; k <= 2 * r; ++k) e += R[(size_t)k * W];
    energy[(size_t)b * H * W + q] = make_float2((float)e, (float)sqrt(e));
}

// The correlation with fused scores and arg-extrema.  Workgroup (tile blockIdx.x, template group blockIdx.y, chunk alignment
// blockIdx.z); lane = column, wavefront w = rows 8w .. 8w + 7 of the tile.  LDS: the tile's padded image, (TH + 2r) x pitch.
__global__ __launch_bounds__(256) void k_epi_match(EdsArrays A, int first, int r, int pitch, const float* __restrict__ pad,
                                                   const float2* __restrict__ energy, const int2* __restrict__ taps,
                                                   const float4* __restrict__ tmeta, unsigned long long* __restrict__ best) {
    extern __shared__ float s_img[];
    const int b = blockIdx.z, slot = first + b, tid = threadIdx.x, H = A.H, W = A.W;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const int g0 = blockIdx.y * EDS_EPI_GROUP;
    if (g0 >= N) return;
    const int g1 = min(N, g0 + EDS_EPI_GROUP);
    const int ntx = (W + EDS_EPI_TW - 1) / EDS_EPI_TW;
    const int tx0 = (blockIdx.x % ntx) * EDS_EPI_TW, ty0 = (blockIdx.x / ntx) * EDS_EPI_TH;
    const int Wp2 = W + 2 * r, Hp2 = H + 2 * r, K = (2 * r + 1) * (2 * r + 1);
    const float* __restrict__ P = pad + (size_t)b * Hp2 * Wp2;
    const int rows = EDS_EPI_TH + 2 * r;
    for (int q = tid; q < rows * pitch; q += 256) {
        const int ly = q / pitch, lx = q - ly * pitch;
        const int gy = ty0 + ly, gx = tx0 + lx;
        s_img[q] = (gy < Hp2 && gx < Wp2) ? P[(size_t)gy * Wp2 + gx] : 0.0f;
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int x = tx0 + lane, yb = ty0 + wave * EDS_EPI_ROWS;
    float e[EDS_EPI_ROWS], se[EDS_EPI_ROWS];
    const float2* __restrict__ En = energy + (size_t)b * H * W;
#pragma unroll
    for (int k = 0; k < EDS_EPI_ROWS; ++k) {
        const bool ok = x < W && yb + k < H;
        const float2 v = ok ? En[(size_t)(yb + k) * W + x] : make_float2(0.0f, 0.0f);
        e[k] = v.x; se[k] = v.y;
    }
    __syncthreads();
    const float* __restrict__ L = s_img + wave * EDS_EPI_ROWS * pitch + lane;
    for (int t = g0; t < g1; ++t) {
        const size_t tt = (size_t)b * A.Np + t;
        const float4 mt = tmeta[tt];
        const int nnz = __float_as_int(mt.x);
        const float S = mt.y, sS = mt.z;
        const int2* __restrict__ T = taps + tt * K;
        float acc[EDS_EPI_ROWS];
#pragma unroll
        for (int k = 0; k < EDS_EPI_ROWS; ++k) acc[k] = 0.0f;
        for (int j = 0; j < nnz; ++j) {
            const int2 tv = T[j];
            const float v = __int_as_float(tv.y);
            const float* __restrict__ Lp = L + tv.x;
#pragma unroll
            for (int k = 0; k < EDS_EPI_ROWS; ++k) acc[k] = fmaf(Lp[k * pitch], v, acc[k]);
        }
        // the normed scores (OpenCV's common_matchTemplate rule) and this lane's arg-extrema, first index on a tie
        unsigned long long kssd = ~0ull, kncc = ~0ull;
#pragma unroll
        for (int k = 0; k < EDS_EPI_ROWS; ++k) {
            if (x >= W || yb + k >= H) continue;
            const float C = acc[k], tn = se[k] * sS;
            const float rt = __builtin_amdgcn_rcpf(tn);
            const float aC = fabsf(C);
            const float cc = aC < tn ? C * rt : (aC < 1.125f * tn ? (C > 0.0f ? 1.0f : -1.0f) : 0.0f);
            float num = (e[k] - 2.0f * C) + S;
            num = num < 0.0f ? 0.0f : num;                  // MAX(num, 0): a NaN stays NaN
            const float sd = num < tn ? num * rt : 1.0f;
            const unsigned long long idx = (unsigned long long)((yb + k) * W + x);
            if (isfinite(sd)) { const unsigned long long kk = ((unsigned long long)ord_key(sd) << 32) | idx; kssd = kk < kssd ? kk : kssd; }
            if (isfinite(cc)) { const unsigned long long kk = ((unsigned long long)(~ord_key(cc)) << 32) | idx; kncc = kk < kncc ? kk : kncc; }
        }
        kssd = wave_min64(kssd);
        kncc = wave_min64(kncc);
        if (lane == 0) {
            unsigned long long* dst = best + 2 * ((size_t)slot * A.Np + t);
            if (kssd != ~0ull) atomicMin(dst, kssd);
            if (kncc != ~0ull) atomicMin(dst + 1, kncc);
        }
    }
}

// per original point: locations and scores from the keys, the cull in fp64 (Tracker.cpp:532)
__global__ __launch_bounds__(256) void k_epi_finish(EdsArrays A, int first, const unsigned long long* __restrict__ best, int32_t* __restrict__ loc,
                                                    double* __restrict__ score, double* __restrict__ ef_tmp, unsigned char* __restrict__ erase) {
    const int slot = first + blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, W = A.W;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (i >= N) return;
    const size_t o = (size_t)slot * A.Np + i;
    const unsigned long long ks = best[2 * o], kn = best[2 * o + 1];
    int sx = -1, sy = -1, nx = -1, ny = -1;
    double ssd = __builtin_nan(""), ncc = __builtin_nan("");
    if (ks != ~0ull) { const unsigned id = (unsigned)ks; sx = (int)(id % (unsigned)W); sy = (int)(id / (unsigned)W); ssd = ord_val((unsigned)(ks >> 32)); }
    if (kn != ~0ull) { const unsigned id = (unsigned)kn; nx = (int)(id % (unsigned)W); ny = (int)(id / (unsigned)W); ncc = ord_val(~(unsigned)(kn >> 32)); }
    loc[4 * o] = sx; loc[4 * o + 1] = sy; loc[4 * o + 2] = nx; loc[4 * o + 3] = ny;
    score[2 * o] = ssd; score[2 * o + 1] = ncc;
    ef_tmp[2 * o] = (double)sx; ef_tmp[2 * o + 1] = (double)sy;
    // cv::norm(Point2d) = sqrt(x x + y y)
    const double ds = sqrt((double)sx * sx + (double)sy * sy), dn = sqrt((double)nx * nx + (double)ny * ny);
    erase[o] = (fabs(ds - dn) > 5.0 || ks == ~0ull || kn == ~0ull) ? 1 : 0;
}

// the ef plane of the kept points (kept == null: every point, in place)
__global__ __launch_bounds__(256) void k_epi_gather(EdsArrays A, int first, const int* __restrict__ kept, const double* __restrict__ ef_tmp,
                                                    double* __restrict__ ef) {
    const int slot = first + blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (k >= N) return;
    const size_t base = (size_t)slot * A.Np, plane = (size_t)A.B * A.Np;
    const int src = kept ? kept[base + k] : k;
    ef[base + k] = ef_tmp[2 * (base + src)];
    ef[plane + base + k] = ef_tmp[2 * (base + src) + 1];
}

// the ef plane as eds_depth_update's EF_COORD input: [count][Np][2], b relative to first
__global__ __launch_bounds__(256) void k_epi_to_aos(EdsArrays A, int first, const double* __restrict__ ef, double* __restrict__ out) {
    const int b = blockIdx.y, slot = first + b, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= A.Np) return;
    const size_t o = (size_t)slot * A.Np + k, plane = (size_t)A.B * A.Np, d = (size_t)b * A.Np + k;
    out[2 * d] = ef[o];
    out[2 * d + 1] = ef[plane + o];
}

template <typename T>
int grow(eds_trk* h, T*& p, size_t& cap, size_t n) {
    if (cap >= n || h->own.regrow(cap, n, {{(void**)&p, n * sizeof(T)}})) return EDS_OK;
    return fail(EDS_ERR_HIP, "allocation of the epiline work buffers failed");
}

int ensure(eds_trk* h) {
    EdsEpiBuffers& e = h->epi;
    if (e.ef) return EDS_OK;
    const size_t B = (size_t)h->B, Np = (size_t)h->Np, H = (size_t)h->H, W = (size_t)h->W;
    if (!h->own.alloc({{(void**)&e.ef, 2 * B * Np * 8}, {(void**)&e.kpix, 2 * B * Np * 8}, {(void**)&e.mval, B * Np * 8},
                       {(void**)&e.keys_tmp, B * Np * 8}, {(void**)&e.keys, B * Np * 8}, {(void**)&e.row_start, B * (H + 2) * 4},
                       {(void**)&e.model, B * H * W * 8}, {(void**)&e.par, B * EDS_EPI_PAR * 8}, {(void**)&e.best, 2 * B * Np * 8},
                       {(void**)&e.ef_tmp, 2 * B * Np * 8}, {(void**)&e.loc, 4 * B * Np * 4}, {(void**)&e.score, 2 * B * Np * 8},
                       {(void**)&e.erase, B * Np}, {(void**)&e.coord, 2 * B * Np * 8}, {(void**)&e.kept, B * Np * 4},
                       {(void**)&e.ef_aos, 2 * B * Np * 8}, pinned(e.h_par, B * EDS_EPI_PAR * 8)}))
        return fail(EDS_ERR_HIP, "allocation of the epiline buffers failed");
    EDS_HIP_TRY(hipMemsetAsync(e.ef, 0, 2 * B * Np * 8, h->own.st));
    return EDS_OK;
}

// getModel of slots first .. first + count - 1 into the model plane
int build_model(eds_trk* h, int first, int count) {
    EdsEpiBuffers& e = h->epi;
    for (int s = first; s < first + count; ++s) {
        const Slot& sl = h->slots[s];
        double* P = e.h_par + (size_t)s * EDS_EPI_PAR;
        for (int j = 0; j < 4; ++j) P[j] = sl.K[j];
        for (int j = 0; j < 6; ++j) P[4 + j] = sl.v[j];          // linearVelocity = vx[0:3], angularVelocity = vx[3:6]
        P[10] = sl.seeded ? 1.0 : 0.0;
    }
    EDS_HIP_TRY(hipMemcpyAsync(e.par + (size_t)first * EDS_EPI_PAR, e.h_par + (size_t)first * EDS_EPI_PAR, (size_t)count * EDS_EPI_PAR * 8,
                               hipMemcpyHostToDevice, h->own.st));
    hipLaunchKernelGGL(k_epi_values, dim3(count), dim3(EDS_EPI_VAL_THREADS), 0, h->own.st, h->arrays(), first, e.par, h->depth.seeds, e.kpix, e.mval);
    EDS_HIP_TRY(hipGetLastError());
    int rc = eds_klt_bin_launch(h, first, count, e.kpix, e.keys_tmp, e.keys, e.row_start, 1);
    if (rc) return rc;
    double k0, k1;
    gauss3_sigma_half(k0, k1);
    const int tiles = ((h->W + EDS_EPI_MODEL_TW - 1) / EDS_EPI_MODEL_TW) * ((h->H + EDS_EPI_MODEL_TH - 1) / EDS_EPI_MODEL_TH);
    hipLaunchKernelGGL(k_epi_model, dim3(tiles, count), dim3(256), 0, h->own.st, h->arrays(), first, k0, k1, k0, e.kpix, e.mval, e.keys, e.row_start,
                       e.model);
    EDS_HIP_TRY(hipGetLastError());
    return EDS_OK;
}

int track(eds_trk* h, int first, int count, int r, int border, int bval, int erase, int stride, int32_t* ssd_xy, int32_t* ncc_xy,
          double* scores, double* ef_xy, int32_t* kept_index, int* n_kept) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (r < 0 || r > EDS_EPI_MAX_RADIUS) return fail(EDS_ERR_INVALID, "patch_radius outside 0 .. 15");
    if (border != EDS_EPI_BORDER_CONSTANT && border != EDS_EPI_BORDER_REPLICATE && border != EDS_EPI_BORDER_REFLECT &&
        border != EDS_EPI_BORDER_REFLECT_101)
        return fail(EDS_ERR_INVALID, "unknown border type");
    if (bval < 0 || bval > 255) return fail(EDS_ERR_INVALID, "border_value outside 0 .. 255");
    if (erase != 0 && erase != 1) return fail(EDS_ERR_INVALID, "erase must be 0 or 1");
    if ((ssd_xy || ncc_xy || scores || ef_xy || kept_index) && stride < max_points(h, first, count))
        return fail(EDS_ERR_INVALID, "stride smaller than the largest point count");
    if ((rc = check_idle_slots(h, first, count, EDS_NEED_KF | EDS_NEED_FRAME))) return rc;
    const int pitch = EDS_EPI_TW + 2 * r;
    const size_t match_lds = (size_t)(EDS_EPI_TH + 2 * r) * pitch * 4;
    size_t max_lds = 0;
    if ((rc = workgroup_lds_limit(h, &max_lds))) return rc;
    if (!row_bins_fit(h, max_lds) || match_lds > max_lds || (size_t)h->H * h->W >= (1ull << 32))
        return fail(EDS_ERR_NOT_USABLE, "the row bins or the match tile of this frame size do not fit the workgroup's LDS");
    if ((rc = ensure(h))) return rc;
    EdsEpiBuffers& e = h->epi;
    const int H = h->H, W = h->W, K = (2 * r + 1) * (2 * r + 1);
    const size_t Np = (size_t)h->Np, Hp2 = (size_t)H + 2 * r, Wp2 = (size_t)W + 2 * r;
    const int cap = std::min(count, EDS_EPI_CHUNK);
    if ((rc = grow(h, e.pad, e.pad_cap, cap * Hp2 * Wp2)) || (rc = grow(h, e.rowsq, e.rowsq_cap, cap * Hp2 * W)) ||
        (rc = grow(h, e.energy, e.energy_cap, (size_t)cap * H * W)) || (rc = grow(h, e.taps, e.taps_cap, cap * Np * K)) ||
        (rc = grow(h, e.tmeta, e.tmeta_cap, cap * Np)))
        return rc;
    const int maxN = max_points(h, first, count);
    // 1. the model images
    if ((rc = build_model(h, first, count))) return rc;
    EDS_HIP_TRY(hipMemsetAsync(e.best + 2 * Np * first, 0xff, 2 * Np * count * 8, h->own.st));
    // 2 .. 4, a chunk of alignments at a time
    const int ntiles = ((W + EDS_EPI_TW - 1) / EDS_EPI_TW) * ((H + EDS_EPI_TH - 1) / EDS_EPI_TH);
    const int ngroups = (maxN + EDS_EPI_GROUP - 1) / EDS_EPI_GROUP;
    for (int c0 = 0; c0 < count; c0 += cap) {
        const int cn = std::min(cap, count - c0), f = first + c0;
        hipLaunchKernelGGL(k_epi_templates, dim3(maxN, cn), dim3(64), 0, h->own.st, h->arrays(), f, r, border, (double)bval, pitch, e.kpix, e.model,
                           e.taps, e.tmeta);
        hipLaunchKernelGGL(k_epi_pad, dim3((unsigned)((Hp2 * Wp2 + 255) / 256), cn), dim3(256), 0, h->own.st, h->arrays(), f, r, border, (float)bval,
                           e.pad);
        hipLaunchKernelGGL(k_epi_rowsq, dim3((unsigned)((Hp2 * W + 255) / 256), cn), dim3(256), 0, h->own.st, H, W, r, e.pad, e.rowsq);
        hipLaunchKernelGGL(k_epi_energy, dim3((unsigned)(((size_t)H * W + 255) / 256), cn), dim3(256), 0, h->own.st, H, W, r, e.rowsq, e.energy);
        hipLaunchKernelGGL(k_epi_match, dim3(ntiles, ngroups, cn), dim3(256), match_lds, h->own.st, h->arrays(), f, r, pitch, e.pad, e.energy, e.taps,
                           e.tmeta, reinterpret_cast<unsigned long long*>(e.best));
        EDS_HIP_TRY(hipGetLastError());
    }
    const unsigned nchunk = (unsigned)((maxN + 255) / 256);
    hipLaunchKernelGGL(k_epi_finish, dim3(nchunk, count), dim3(256), 0, h->own.st, h->arrays(), first,
                       reinterpret_cast<const unsigned long long*>(e.best), e.loc, e.score, e.ef_tmp, e.erase);
    EDS_HIP_TRY(hipGetLastError());
    // the per-original-point outputs, before the compaction
    std::vector<int32_t> vloc;
    std::vector<double> vsc;
    if (ssd_xy || ncc_xy) { vloc.resize(4 * Np * count); EDS_HIP_TRY(hipMemcpyAsync(vloc.data(), e.loc + 4 * Np * first, vloc.size() * 4, hipMemcpyDeviceToHost, h->own.st)); }
    if (scores) { vsc.resize(2 * Np * count); EDS_HIP_TRY(hipMemcpyAsync(vsc.data(), e.score + 2 * Np * first, vsc.size() * 8, hipMemcpyDeviceToHost, h->own.st)); }
    std::vector<int> n0(count);
    for (int b = 0; b < count; ++b) n0[b] = h->slots[first + b].N;
    // 5. the cull: getCoord's compaction, erasing by flag
    if (erase) {
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
        const EdsPointsDev dev = {e.coord, e.kept, e.erase};
        if ((rc = update_points_range(h, first, count, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &dev))) return rc;
    }
    hipLaunchKernelGGL(k_epi_gather, dim3(nchunk, count), dim3(256), 0, h->own.st, h->arrays(), first, erase ? e.kept : nullptr, e.ef_tmp, e.ef);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<int32_t> vk;
    if (kept_index && erase) { vk.resize(Np * count); EDS_HIP_TRY(hipMemcpyAsync(vk.data(), e.kept + Np * first, Np * count * 4, hipMemcpyDeviceToHost, h->own.st)); }
    if (ef_xy && (rc = read_xy_planes(h, e.ef, first, count, stride, ef_xy))) return rc;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    for (int b = 0; b < count; ++b) {
        Slot& sl = h->slots[first + b];
        sl.epi_valid = sl.has_kf && sl.N > 0;
        const int nk = sl.N;
        const size_t o = (size_t)b * stride, src = Np * b;
        if (n_kept) n_kept[b] = nk;
        for (int i = 0; i < n0[b]; ++i) {
            if (ssd_xy) { ssd_xy[2 * (o + i)] = vloc[4 * (src + i)]; ssd_xy[2 * (o + i) + 1] = vloc[4 * (src + i) + 1]; }
            if (ncc_xy) { ncc_xy[2 * (o + i)] = vloc[4 * (src + i) + 2]; ncc_xy[2 * (o + i) + 1] = vloc[4 * (src + i) + 3]; }
            if (scores) { scores[2 * (o + i)] = vsc[2 * (src + i)]; scores[2 * (o + i) + 1] = vsc[2 * (src + i) + 1]; }
        }
        for (int k = 0; kept_index && k < nk; ++k) kept_index[o + k] = erase ? vk[src + k] : k;
    }
    return EDS_OK;
}

}  // namespace

extern "C" {

int eds_epi_abi_version(void) { return EDS_HIP_EPILINE_ABI_VERSION; }

int eds_epi_track_points(eds_trk* h, int first, int count, int patch_radius, int border_type, int border_value, int erase, int stride,
                         int32_t* ssd_xy, int32_t* ncc_xy, double* scores, double* ef_xy, int32_t* kept_index, int* n_kept) {
    return track(h, first, count, patch_radius, border_type, border_value, erase, stride, ssd_xy, ncc_xy, scores, ef_xy, kept_index, n_kept);
}

int eds_epi_get(eds_trk* h, int slot, double* ef_xy) {
    int rc = check_slot(h, slot);
    if (rc) return rc;
    if (!ef_xy) return fail(EDS_ERR_INVALID, "null output");
    if ((rc = check_idle_slots(h, slot, 1, EDS_NEED_KF))) return rc;
    if (!h->epi.ef || !h->slots[slot].epi_valid) return fail(EDS_ERR_STATE, "the slot's ef plane is not current: run eds_epi_track_points");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    return read_xy_planes(h, h->epi.ef, slot, 1, h->slots[slot].N, ef_xy);
}

int eds_epi_get_model(eds_trk* h, int slot, double* model) {
    int rc = check_slot(h, slot);
    if (rc) return rc;
    if (!model) return fail(EDS_ERR_INVALID, "null output");
    if ((rc = check_idle_slots(h, slot, 1, EDS_NEED_KF))) return rc;
    size_t max_lds = 0;
    if ((rc = workgroup_lds_limit(h, &max_lds))) return rc;
    if (!row_bins_fit(h, max_lds)) return fail(EDS_ERR_NOT_USABLE, "the row bins of this frame size do not fit the workgroup's LDS");
    if ((rc = ensure(h)) || (rc = build_model(h, slot, 1))) return rc;
    const size_t n = (size_t)h->H * h->W;
    EDS_HIP_TRY(hipMemcpyAsync(model, h->epi.model + n * slot, n * 8, hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_epi_depth_update(eds_trk* h, int first, int count, const double* T_kf_ef, int filter, eds_depth_summary* out) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if ((rc = check_idle_slots(h, first, count, 0))) return rc;
    for (int s = first; s < first + count; ++s)
        if (!h->epi.ef || !h->slots[s].epi_valid || !h->slots[s].has_kf)
            return fail(EDS_ERR_STATE, "the slot's ef plane is not current: run eds_epi_track_points");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    hipLaunchKernelGGL(k_epi_to_aos, dim3((h->Np + 255) / 256, count), dim3(256), 0, h->own.st, h->arrays(), first, h->epi.ef, h->epi.ef_aos);
    EDS_HIP_TRY(hipGetLastError());
    return eds_depth_update_impl(h, first, count, EDS_DEPTH_EF_COORD, nullptr, nullptr, 0, T_kf_ef, filter, out, h->epi.ef_aos);
}

}  // extern "C"
