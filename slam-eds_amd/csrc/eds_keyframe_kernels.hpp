// The kernels of the keyframe point set-up (KeyFrame::create, reference KeyFrame.cpp:333-463), shared by the single-slot build
// (eds_keyframe.hip) and the batched keyframe switch (eds_kfswitch.hip).  Every kernel is a __device__ body d_* plus two thin __global__
// entries: k_* for one slot, with its counts passed by value, and k_*_b for a chunk of slots (one more grid dimension), whose counts are
// read from device memory so that nothing waits on the host between them.  Both run the same body on the same values: what the batched
// call leaves in a slot is what the single call leaves there, bit for bit.  Internal linkage: each translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "eds_handle.hpp"
#include "eds_kdtree.hpp"

#pragma clang fp contract(off)      // sums are formed exactly as written (the oracle states the same association)

namespace {

constexpr int KF_T = 256;
constexpr int KF_MAX_CELL = 32;                     // cell^2 <= 1024 magnitudes in LDS
constexpr double KF_LOG_EPS = (double)0.2f;         // `static constexpr float log_eps = 0.2` (KeyFrame.hpp:54)

__device__ __forceinline__ double load_px(const void* img, int type, size_t i) {
    if (type == 0) return (double)static_cast<const uint8_t*>(img)[i];
    if (type == 1) return (double)static_cast<const float*>(img)[i];
    return static_cast<const double*>(img)[i];
}

// ---- image preparation: what KeyFrame::create does to the image before anything else (KeyFrame.cpp:352-362) ----------------------
// (1) `cv::resize(img, img, out_size, cv::INTER_CUBIC)` when out_scale != 1 — INTER_CUBIC lands in the `fx` parameter, so the
//     interpolation is OpenCV's default INTER_LINEAR, replaced by the 2x2 block mean when both scales are exactly 2;
// (2) `cv::cvtColor(img, img, cv::COLOR_RGB2GRAY)` for a colour image.
// Both restated per element type from OpenCV's published implementation (imgproc/resize.cpp, color_rgb.simd.hpp): uint8 runs in
// fixed point (11-bit interpolation weights, 14-bit luma coefficients 4899 / 9617 / 1868), float in fp32, double in fp64.
__device__ __forceinline__ void kf_resize_coord(int d, double scale, int n_src, int* s0, int* s1, float* f) {
    float fr = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(fr);
    fr -= (float)s;
    if (s < 0) { fr = 0.0f; s = 0; }
    if (s >= n_src - 1) { fr = 0.0f; s = n_src - 1; }
    *s0 = s; *s1 = s + 1 < n_src ? s + 1 : n_src - 1; *f = fr;
}
__device__ __forceinline__ int kf_round_short(float v) {               // saturate_cast<short>(float): round half to even, saturate
    const float r = rintf(v);
    return r > 32767.0f ? 32767 : (r < -32768.0f ? -32768 : (int)r);
}
// one channel `ch` of pixel (r, c) of the H x W image resized from src (sH x sW, `cn` interleaved channels)
template <class T>
__device__ __forceinline__ T kf_resized(const T* __restrict__ src, int sH, int sW, int cn, int ch, int H, int W, int r, int c);
template <>
__device__ __forceinline__ uint8_t kf_resized<uint8_t>(const uint8_t* __restrict__ src, int sH, int sW, int cn, int ch, int H, int W, int r, int c) {
    if (sH == H && sW == W) return src[((size_t)r * sW + c) * cn + ch];
    if (sH == 2 * H && sW == 2 * W) {
        const uint8_t* p = src + ((size_t)(2 * r) * sW + 2 * c) * cn + ch;
        return (uint8_t)((p[0] + p[cn] + p[(size_t)sW * cn] + p[(size_t)sW * cn + cn] + 2) >> 2);
    }
    int x0, x1, y0, y1; float fx, fy;
    kf_resize_coord(c, (double)sW / (double)W, sW, &x0, &x1, &fx);
    kf_resize_coord(r, (double)sH / (double)H, sH, &y0, &y1, &fy);
    const int a0 = kf_round_short((1.0f - fx) * 2048.0f), a1 = kf_round_short(fx * 2048.0f);
    const int b0 = kf_round_short((1.0f - fy) * 2048.0f), b1 = kf_round_short(fy * 2048.0f);
    const int S0 = src[((size_t)y0 * sW + x0) * cn + ch] * a0 + src[((size_t)y0 * sW + x1) * cn + ch] * a1;
    const int S1 = src[((size_t)y1 * sW + x0) * cn + ch] * a0 + src[((size_t)y1 * sW + x1) * cn + ch] * a1;
    return (uint8_t)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
}
template <>
__device__ __forceinline__ float kf_resized<float>(const float* __restrict__ src, int sH, int sW, int cn, int ch, int H, int W, int r, int c) {
    if (sH == H && sW == W) return src[((size_t)r * sW + c) * cn + ch];
    if (sH == 2 * H && sW == 2 * W) {
        const float* p = src + ((size_t)(2 * r) * sW + 2 * c) * cn + ch;
        return ((((0.0f + p[0]) + p[cn]) + p[(size_t)sW * cn]) + p[(size_t)sW * cn + cn]) * 0.25f;
    }
    int x0, x1, y0, y1; float fx, fy;
    kf_resize_coord(c, (double)sW / (double)W, sW, &x0, &x1, &fx);
    kf_resize_coord(r, (double)sH / (double)H, sH, &y0, &y1, &fy);
    const float a0 = 1.0f - fx, a1 = fx, b0 = 1.0f - fy, b1 = fy;
    const float S0 = src[((size_t)y0 * sW + x0) * cn + ch] * a0 + src[((size_t)y0 * sW + x1) * cn + ch] * a1;
    const float S1 = src[((size_t)y1 * sW + x0) * cn + ch] * a0 + src[((size_t)y1 * sW + x1) * cn + ch] * a1;
    return S0 * b0 + S1 * b1;
}
template <>
__device__ __forceinline__ double kf_resized<double>(const double* __restrict__ src, int sH, int sW, int cn, int ch, int H, int W, int r, int c) {
    if (sH == H && sW == W) return src[((size_t)r * sW + c) * cn + ch];
    if (sH == 2 * H && sW == 2 * W) {
        const double* p = src + ((size_t)(2 * r) * sW + 2 * c) * cn + ch;
        return ((((0.0 + p[0]) + p[cn]) + p[(size_t)sW * cn]) + p[(size_t)sW * cn + cn]) * 0.25;
    }
    int x0, x1, y0, y1; float fx, fy;
    kf_resize_coord(c, (double)sW / (double)W, sW, &x0, &x1, &fx);
    kf_resize_coord(r, (double)sH / (double)H, sH, &y0, &y1, &fy);
    const double a0 = (double)(1.0f - fx), a1 = (double)fx, b0 = (double)(1.0f - fy), b1 = (double)fy;
    const double S0 = src[((size_t)y0 * sW + x0) * cn + ch] * a0 + src[((size_t)y0 * sW + x1) * cn + ch] * a1;
    const double S1 = src[((size_t)y1 * sW + x0) * cn + ch] * a0 + src[((size_t)y1 * sW + x1) * cn + ch] * a1;
    return S0 * b0 + S1 * b1;
}
template <class T>
__global__ __launch_bounds__(KF_T) void k_prepare(const T* __restrict__ src, int sH, int sW, int cn, T* __restrict__ dst, int H, int W) {
    const int c = blockIdx.x * KF_T + threadIdx.x, r = blockIdx.y;
    if (c >= W) return;
    T v;
    if (cn == 1) {
        v = kf_resized<T>(src, sH, sW, 1, 0, H, W, r, c);
    } else {                            // COLOR_RGB2GRAY on the resized pixel
        const T R = kf_resized<T>(src, sH, sW, cn, 0, H, W, r, c), G = kf_resized<T>(src, sH, sW, cn, 1, H, W, r, c),
                B = kf_resized<T>(src, sH, sW, cn, 2, H, W, r, c);
        if (sizeof(T) == 1) v = (T)(((int)R * 4899 + (int)G * 9617 + (int)B * 1868 + (1 << 13)) >> 14);
        else v = (T)((float)R * 0.299f + (float)G * 0.587f + (float)B * 0.114f);
    }
    dst[(size_t)r * W + c] = v;
}

// block-level min / max; result valid on thread 0
__device__ __forceinline__ void block_minmax(double& mn, double& mx) {
    __shared__ double s_mn[KF_T], s_mx[KF_T];
    s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx;
    __syncthreads();
    for (int s = KF_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_mn[threadIdx.x] = fmin(s_mn[threadIdx.x], s_mn[threadIdx.x + s]);
            s_mx[threadIdx.x] = fmax(s_mx[threadIdx.x], s_mx[threadIdx.x + s]);
        }
        __syncthreads();
    }
    mn = s_mn[0]; mx = s_mx[0];
    __syncthreads();
}

// partial[2 b], partial[2 b + 1] = min, max over block b's grid-stride share  (cv::minMaxLoc, KeyFrame.cpp:365)
__device__ __forceinline__ void d_minmax(const void* img, int type, size_t n, double* partial) {
    double mn = INFINITY, mx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * KF_T + threadIdx.x; i < n; i += (size_t)gridDim.x * KF_T) {
        const double v = load_px(img, type, i);
        mn = fmin(mn, v); mx = fmax(mx, v);
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = mn; partial[2 * blockIdx.x + 1] = mx; }
}
__global__ __launch_bounds__(KF_T) void k_minmax(const void* img, int type, size_t n, double* partial) { d_minmax(img, type, n, partial); }
// slot blockIdx.y of a chunk: its image at img + y * img_stride bytes, its partials at partial + y * partial_stride
__global__ __launch_bounds__(KF_T) void k_minmax_b(const void* img, size_t img_stride, int type, size_t n, double* partial, int partial_stride) {
    d_minmax(static_cast<const char*>(img) + blockIdx.y * img_stride, type, n, partial + (size_t)blockIdx.y * partial_stride);
}
// ... over the first count[y * count_stride] doubles of plane y (the candidates' distances)
__global__ __launch_bounds__(KF_T) void k_minmax_counted_b(const double* plane, size_t plane_stride, const int* __restrict__ count, int count_stride,
                                                            double* partial, int partial_stride) {
    d_minmax(plane + blockIdx.y * plane_stride, 2, (size_t)count[(size_t)blockIdx.y * count_stride], partial + (size_t)blockIdx.y * partial_stride);
}

__device__ __forceinline__ void final_minmax(const double* partial, int nblocks, double& mn, double& mx) {
    mn = INFINITY; mx = -INFINITY;
    for (int b = threadIdx.x; b < nblocks; b += KF_T) { mn = fmin(mn, partial[2 * b]); mx = fmax(mx, partial[2 * b + 1]); }
    block_minmax(mn, mx);
}

// L = log((img - min)/(max - min) + log_eps)   (KeyFrame.cpp:366,373-374)
__device__ __forceinline__ void d_log(const void* img, int type, size_t n, const double* partial, int nblocks, double* L) {
    double mn, mx;
    final_minmax(partial, nblocks, mn, mx);
    const double range = mx - mn;
    for (size_t i = (size_t)blockIdx.x * KF_T + threadIdx.x; i < n; i += (size_t)gridDim.x * KF_T)
        L[i] = log((load_px(img, type, i) - mn) / range + KF_LOG_EPS);
}
__global__ __launch_bounds__(KF_T) void k_log(const void* img, int type, size_t n, const double* partial, int nblocks, double* L) {
    d_log(img, type, n, partial, nblocks, L);
}
__global__ __launch_bounds__(KF_T) void k_log_b(const void* img, size_t img_stride, int type, size_t n, const double* partial, int partial_stride,
                                                 int nblocks, double* L) {
    d_log(static_cast<const char*>(img) + blockIdx.y * img_stride, type, n, partial + (size_t)blockIdx.y * partial_stride, nblocks, L + blockIdx.y * n);
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// cv::Sobel(L, CV_64F, 1, 0, 3) / (0, 1, 3), BORDER_REFLECT_101, and cv::cartToPolar's magnitude  (KeyFrame.cpp:384-401)
__device__ __forceinline__ void d_sobel(const double* __restrict__ L, int H, int W, double* __restrict__ gx,
                                                double* __restrict__ gy, double* __restrict__ mag) {
    const int c = blockIdx.x * KF_T + threadIdx.x, r = blockIdx.y;
    if (c >= W) return;
    const int r0 = reflect101(r - 1, H), r2 = reflect101(r + 1, H), c0 = reflect101(c - 1, W), c2 = reflect101(c + 1, W);
    const double* t = L + (size_t)r0 * W; const double* m = L + (size_t)r * W; const double* b = L + (size_t)r2 * W;
    const double x = ((t[c2] - t[c0]) + 2.0 * (m[c2] - m[c0])) + (b[c2] - b[c0]);
    const double y = ((b[c0] - t[c0]) + 2.0 * (b[c] - t[c])) + (b[c2] - t[c2]);
    const size_t o = (size_t)r * W + c;
    gx[o] = x; gy[o] = y; mag[o] = sqrt(x * x + y * y);
}
__global__ __launch_bounds__(KF_T) void k_sobel(const double* __restrict__ L, int H, int W, double* __restrict__ gx, double* __restrict__ gy,
                                                double* __restrict__ mag) { d_sobel(L, H, W, gx, gy, mag); }

// cv::Sobel with aperture 7 (the KeyFrame constructor's, reference KeyFrame.cpp:239-240): separable kernels smooth = [1 6 15 20 15 6 1],
// derivative = [-1 -4 -5 0 5 4 1] (cv::getSobelKernels), no scale, reflect-101 border, CV_64F — the row pass first, then the column
// pass, each in the order OpenCV's symmetric / anti-symmetric filters add: centre term, then the pairs outwards.
__device__ __forceinline__ void d_sobel7(const double* __restrict__ L, int H, int W, double* __restrict__ gx,
                                                 double* __restrict__ gy, double* __restrict__ mag) {
    const int c = blockIdx.x * KF_T + threadIdx.x, r = blockIdx.y;
    if (c >= W) return;
    int cc[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) cc[j] = reflect101(c + j - 3, W);
    double rs[7], rd[7];                       // row pass of the seven rows around r: smoothed / differentiated along x
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double* p = L + (size_t)reflect101(r + k - 3, H) * W;
        rs[k] = ((20.0 * p[cc[3]] + 15.0 * (p[cc[4]] + p[cc[2]])) + 6.0 * (p[cc[5]] + p[cc[1]])) + (p[cc[6]] + p[cc[0]]);
        rd[k] = (5.0 * (p[cc[4]] - p[cc[2]]) + 4.0 * (p[cc[5]] - p[cc[1]])) + (p[cc[6]] - p[cc[0]]);
    }
    const double x = ((20.0 * rd[3] + 15.0 * (rd[4] + rd[2])) + 6.0 * (rd[5] + rd[1])) + (rd[6] + rd[0]);
    const double y = (5.0 * (rs[4] - rs[2]) + 4.0 * (rs[5] - rs[1])) + (rs[6] - rs[0]);
    const size_t o = (size_t)r * W + c;
    gx[o] = x; gy[o] = y; mag[o] = sqrt(x * x + y * y);
}
__global__ __launch_bounds__(KF_T) void k_sobel7(const double* __restrict__ L, int H, int W, double* __restrict__ gx, double* __restrict__ gy,
                                                 double* __restrict__ mag) { d_sobel7(L, H, W, gx, gy, mag); }
// slot blockIdx.z of a chunk: planes H * W doubles apart
__global__ __launch_bounds__(KF_T) void k_sobel_b(int ksize, const double* __restrict__ L, int H, int W, double* __restrict__ gx,
                                                  double* __restrict__ gy, double* __restrict__ mag) {
    const size_t o = (size_t)blockIdx.z * H * W;
    if (ksize == 7) d_sobel7(L + o, H, W, gx + o, gy + o, mag + o);
    else d_sobel(L + o, H, W, gx + o, gy + o, mag + o);
}

// One workgroup per cell.  cand[cellid][pos] = local index (row-major inside the cell) in the reference's push order.
// The cell's magnitudes (>= 0, so their bit patterns order like the values) are SORTED once — bitonic network in LDS over (magnitude
// descending, index ascending): position p then holds the element of descending rank p, exact ties resolved by index like the
// reference's repeated arg-max — instead of every element counting its rank against all others (O(n^2) fp64 compares: 44 us for a VGA
// image in 20 x 20 cells; this: ~12 us).
__device__ __forceinline__ void d_select(const double* __restrict__ mag, int W, int cell, int ncx, int method, int k_per_cell,
                                         int* __restrict__ cand, int* __restrict__ cnt) {
    constexpr int MAXN = KF_MAX_CELL * KF_MAX_CELL;
    __shared__ unsigned long long v[MAXN];          // bits of the magnitudes, row-major inside the cell
    __shared__ unsigned long long key[MAXN];        // ... sorted
    __shared__ unsigned short idx[MAXN];
    __shared__ int s_count, s_wave[KF_T / 64], s_base;
    const int n2 = cell * cell, tid = threadIdx.x;
    const int cy = blockIdx.x / ncx, cx = blockIdx.x - cy * ncx;
    const int x0 = cx * cell, y0 = cy * cell;
    int M = 2;
    while (M < n2) M <<= 1;
    for (int i = tid; i < M; i += KF_T) {
        const unsigned long long k = i < n2 ? (unsigned long long)__double_as_longlong(mag[(size_t)(y0 + i / cell) * W + x0 + i % cell]) : 0ull;
        if (i < n2) v[i] = k;
        key[i] = k; idx[i] = (unsigned short)i;     // padding: magnitude 0 with an index beyond the cell's: sorts behind every real element
    }
    if (tid == 0) { s_count = 0; s_base = 0; }
    __syncthreads();
    for (int k = 2; k <= M; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < M; i += KF_T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long ka = key[i], kb = key[ixj];
                    const unsigned short ia = idx[i], ib = idx[ixj];
                    const bool b_first = (kb > ka) || (kb == ka && ib < ia);      // b belongs in front of a
                    if (b_first == ((i & k) == 0)) { key[i] = kb; key[ixj] = ka; idx[i] = ib; idx[ixj] = ia; }
                }
            }
            __syncthreads();
        }
    }
    int* out = cand + (size_t)blockIdx.x * n2;
    int mine = 0;
    if (method == 1) {                       // MEDIAN: every magnitude above the cell median, row-major order (:797-817)
        const unsigned long long med = key[n2 - 1 - n2 / 2];                      // nth_element(size / 2): ascending position n2 / 2  (Utils.cpp:497-498)
        for (int c0 = 0; c0 < n2; c0 += KF_T) {
            const int i = c0 + tid;
            const bool pick = i < n2 && v[i] > med;
            const unsigned long long bal = __ballot(pick);
            const int lane = tid & 63, wave = tid >> 6;
            if (lane == 0) s_wave[wave] = __popcll(bal);
            __syncthreads();
            int before = s_base;
            for (int w = 0; w < wave; ++w) before += s_wave[w];
            if (pick) { out[before + __popcll(bal & ((1ull << lane) - 1ull))] = i; ++mine; }
            __syncthreads();
            if (tid == 0) { int t = 0; for (int w = 0; w < KF_T / 64; ++w) t += s_wave[w]; s_base += t; }
            __syncthreads();
        }
    } else {                                 // MAX: k times arg-max-and-zero; stops once the rest is flat (:768-793)
        const bool flat = key[0] == key[n2 - 1];                                  // max == min: nothing to pick (:784)
        const int kk = k_per_cell < n2 ? k_per_cell : n2;
        for (int p = tid; p < kk; p += KF_T)
            if (!flat && key[p] != 0ull) { out[p] = idx[p]; ++mine; }            // magnitude > 0
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = s_count;
}
__global__ __launch_bounds__(KF_T) void k_select(const double* __restrict__ mag, int W, int cell, int ncx, int method, int k_per_cell,
                                                 int* __restrict__ cand, int* __restrict__ cnt) {
    d_select(mag, W, cell, ncx, method, k_per_cell, cand, cnt);
}
// slot blockIdx.y of a chunk: planes npx elements apart, cell counts and offsets cell_stride ints apart
__global__ __launch_bounds__(KF_T) void k_select_b(const double* __restrict__ mag, size_t npx, int W, int cell, int ncx, int method, int k_per_cell,
                                                   int* __restrict__ cand, int* __restrict__ cnt, int cell_stride) {
    d_select(mag + blockIdx.y * npx, W, cell, ncx, method, k_per_cell, cand + blockIdx.y * npx, cnt + (size_t)blockIdx.y * cell_stride);
}

// exclusive scan of the per-cell counts (single workgroup); off[ncell] = total
__device__ __forceinline__ void d_scan_cells(const int* __restrict__ cnt, int ncell, int* __restrict__ off) {
    __shared__ int s[KF_T];
    __shared__ int s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < ncell; base += KF_T) {
        const int i = base + threadIdx.x;
        const int c = i < ncell ? cnt[i] : 0;
        s[threadIdx.x] = c;
        __syncthreads();
        for (int d = 1; d < KF_T; d <<= 1) {
            const int t = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < ncell) off[i] = s_run + s[threadIdx.x] - c;
        __syncthreads();
        if (threadIdx.x == KF_T - 1) s_run += s[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) off[ncell] = s_run;
}
__global__ __launch_bounds__(KF_T) void k_scan_cells(const int* __restrict__ cnt, int ncell, int* __restrict__ off) { d_scan_cells(cnt, ncell, off); }
__global__ __launch_bounds__(KF_T) void k_scan_cells_b(const int* __restrict__ cnt, int ncell, int* __restrict__ off, int cell_stride) {
    d_scan_cells(cnt + (size_t)blockIdx.x * cell_stride, ncell, off + (size_t)blockIdx.x * cell_stride);
}

// candidate pixel coordinates and their Sobel gradient, in push order  (KeyFrame.cpp:413-430)
__device__ __forceinline__ void d_emit(const int* __restrict__ cand, const int* __restrict__ cnt, const int* __restrict__ off,
                                       int cell, int ncx, int W, const double* __restrict__ gx, const double* __restrict__ gy,
                                       double* __restrict__ coord, double* __restrict__ grad) {
    const int cid = blockIdx.x;
    const int n2 = cell * cell, c = cnt[cid], o = off[cid];
    const int cy = cid / ncx, cx = cid - cy * ncx;
    for (int p = threadIdx.x; p < c; p += KF_T) {
        const int li = cand[(size_t)cid * n2 + p];
        const int x = cx * cell + li % cell, y = cy * cell + li / cell;
        coord[2 * (size_t)(o + p)] = (double)x; coord[2 * (size_t)(o + p) + 1] = (double)y;
        grad[2 * (size_t)(o + p)] = gx[(size_t)y * W + x]; grad[2 * (size_t)(o + p) + 1] = gy[(size_t)y * W + x];
    }
}
__global__ __launch_bounds__(KF_T) void k_emit(const int* __restrict__ cand, const int* __restrict__ cnt, const int* __restrict__ off,
                                               int cell, int ncx, int W, const double* __restrict__ gx, const double* __restrict__ gy,
                                               double* __restrict__ coord, double* __restrict__ grad) {
    d_emit(cand, cnt, off, cell, ncx, W, gx, gy, coord, grad);
}
__global__ __launch_bounds__(KF_T) void k_emit_b(const int* __restrict__ cand, const int* __restrict__ cnt, const int* __restrict__ off, int cell_stride,
                                                 size_t npx, int cell, int ncx, int W, const double* __restrict__ gx, const double* __restrict__ gy,
                                                 double* __restrict__ coord, double* __restrict__ grad) {
    const size_t y = blockIdx.y;
    d_emit(cand + y * npx, cnt + y * cell_stride, off + y * cell_stride, cell, ncx, W, gx + y * npx, gy + y * npx, coord + 2 * y * npx, grad + 2 * y * npx);
}

// Nearest depth-map point of every candidate (KeyFrame.cpp:1137-1166): the reference's k-d tree, built on the host with
// std::nth_element (eds_kdtree.hpp), walked here one candidate per lane with an explicit stack.  The tree's nodes come in tree order
// (txy, tidp), so the winner's position reads its idp directly.  Distances are fp64 sqrt of separately rounded squares and sum, and a
// strict `<` in the reference's traversal order decides: an exact tie goes to the first point of that traversal, which depends on
// libstdc++'s nth_element (pinned for this toolchain by tests/test_kdtree_pin.py).
__device__ __forceinline__ void d_nearest_tree(const double* __restrict__ coord, int n, const double* __restrict__ txy,
                                               const double* __restrict__ tidp, int m, double* __restrict__ idp, double* __restrict__ dist) {
    const int i = blockIdx.x * KF_T + threadIdx.x;
    if (i >= n) return;
    const double qx = coord[2 * (size_t)i], qy = coord[2 * (size_t)i + 1];
    const int k = edskd::nn(txy, m, qx, qy, nullptr);
    const double dx = txy[2 * (size_t)k] - qx, dy = txy[2 * (size_t)k + 1] - qy;      // cv::norm(dist)  (:1161-1162)
    idp[i] = tidp[k];
    dist[i] = sqrt(dx * dx + dy * dy);
}
__global__ __launch_bounds__(KF_T) void k_nearest_tree(const double* __restrict__ coord, int n, const double* __restrict__ txy,
                                                       const double* __restrict__ tidp, int m, double* __restrict__ idp, double* __restrict__ dist) {
    d_nearest_tree(coord, n, txy, tidp, m, idp, dist);
}
// slot blockIdx.y of a chunk: n = the candidate count the scan left, m = the map's size, both read here; a slot without a map, or whose
// tree the device did not build (tree_flag != 0: the host redoes that slot), is skipped
__global__ __launch_bounds__(KF_T) void k_nearest_tree_b(const double* __restrict__ coord, size_t npx, const int* __restrict__ ncand, int cell_stride,
                                                         const double* __restrict__ txy, const double* __restrict__ tidp, size_t map_stride,
                                                         const int* __restrict__ map_n, const int* __restrict__ tree_flag,
                                                         double* __restrict__ idp, double* __restrict__ dist) {
    const size_t y = blockIdx.y;
    const int m = map_n[y];
    if (m < 1 || tree_flag[y] != 0) return;
    d_nearest_tree(coord + 2 * y * npx, ncand[y * cell_stride], txy + 2 * y * map_stride, tidp + y * map_stride, m, idp + y * npx, dist + y * npx);
}

// weights from the distances (:1168-1181), cleanPoints(thr) (:1566-1587): in-place, order-preserving compaction.
// Single workgroup; a chunk is read completely before it is written, and destinations never pass the read front.
__device__ __forceinline__ void d_weights_clean(double* __restrict__ coord, double* __restrict__ grad, double* __restrict__ idp,
                                                double* __restrict__ wd, int n, int has_depth, double const_idp,
                                                const double* __restrict__ partial, int nblocks, double thr, int* __restrict__ summary) {
    __shared__ double s_mn[1024], s_mx[1024];
    __shared__ int s_wave[16];
    __shared__ int s_run;
    double mn = INFINITY, mx = -INFINITY;
    if (has_depth) {
        for (int b = threadIdx.x; b < nblocks; b += 1024) { mn = fmin(mn, partial[2 * b]); mx = fmax(mx, partial[2 * b + 1]); }
        s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx;
        __syncthreads();
        for (int s = 512; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                s_mn[threadIdx.x] = fmin(s_mn[threadIdx.x], s_mn[threadIdx.x + s]);
                s_mx[threadIdx.x] = fmax(s_mx[threadIdx.x], s_mx[threadIdx.x + s]);
            }
            __syncthreads();
        }
        mn = s_mn[0]; mx = s_mx[0];
    }
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        double w = 1.0, c0 = 0, c1 = 0, g0 = 0, g1 = 0, d = const_idp;
        bool keep = false;
        if (i < n) {
            if (has_depth) {
                if (mn != mx) w = 1.0 - ((wd[i] - mn) / (mx - mn));
                d = idp[i];
            }
            keep = !(w < thr);
            c0 = coord[2 * (size_t)i]; c1 = coord[2 * (size_t)i + 1]; g0 = grad[2 * (size_t)i]; g1 = grad[2 * (size_t)i + 1];
        }
        const unsigned long long bal = __ballot(keep);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < 16; ++k) { const int c = s_wave[k]; before += k < wave ? c : 0; total += c; }
        const int run = s_run;
        if (keep) {
            const size_t o = (size_t)(run + before + within);
            coord[2 * o] = c0; coord[2 * o + 1] = c1; grad[2 * o] = g0; grad[2 * o + 1] = g1; idp[o] = d; wd[o] = w;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_run = run + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) { summary[0] = n; summary[1] = s_run; }
}
__global__ __launch_bounds__(1024) void k_weights_clean(double* __restrict__ coord, double* __restrict__ grad, double* __restrict__ idp,
                                                        double* __restrict__ wd, int n, int has_depth, double const_idp,
                                                        const double* __restrict__ partial, int nblocks, double thr, int* __restrict__ summary) {
    d_weights_clean(coord, grad, idp, wd, n, has_depth, const_idp, partial, nblocks, thr, summary);
}
// slot blockIdx.x of a chunk; summary: 4 ints per slot {candidates, kept, map size, tree flag}
__global__ __launch_bounds__(1024) void k_weights_clean_b(double* __restrict__ coord, double* __restrict__ grad, double* __restrict__ idp,
                                                          double* __restrict__ wd, size_t npx, const int* __restrict__ ncand, int cell_stride,
                                                          const int* __restrict__ map_n, const int* __restrict__ tree_flag, double const_idp,
                                                          const double* __restrict__ partial, int partial_stride, int nblocks, double thr,
                                                          int* __restrict__ summary) {
    const size_t y = blockIdx.x;
    d_weights_clean(coord + 2 * y * npx, grad + 2 * y * npx, idp + y * npx, wd + y * npx, ncand[y * cell_stride], map_n[y] > 0 ? 1 : 0, const_idp,
                    partial + y * partial_stride, nblocks, thr, summary + 4 * y);
    if (threadIdx.x == 0) { summary[4 * y + 2] = map_n[y]; summary[4 * y + 3] = tree_flag[y]; }
}

// the slot's fp32 planes from the cleaned fp64 arrays — the same conversion set_keyframe does on the host
__device__ __forceinline__ void d_fill_slot(const EdsArrays& A, int slot, int N, double fx, double fy, double cx, double cy,
                                            const double* __restrict__ coord, const double* __restrict__ grad,
                                            const double* __restrict__ idp, const double* __restrict__ w) {
    const int i = blockIdx.x * KF_T + threadIdx.x;
    if (i >= A.Np) return;
    const size_t o = (size_t)slot * A.Np + i;
    const bool in = i < N;
    const double nx = in ? (coord[2 * (size_t)i] - cx) / fx : 0.0, ny = in ? (coord[2 * (size_t)i + 1] - cy) / fy : 0.0;   // :417-423
    const_cast<float*>(A.x)[o] = (float)nx;
    const_cast<float*>(A.y)[o] = (float)ny;
    const_cast<float*>(A.rho)[o] = in ? (float)idp[i] : 1.f;
    const_cast<float*>(A.gx)[o] = in ? (float)grad[2 * (size_t)i] : 0.f;
    const_cast<float*>(A.gy)[o] = in ? (float)grad[2 * (size_t)i + 1] : 0.f;
    const_cast<float*>(A.w)[o] = in ? (float)w[i] : 0.f;
    const double u0 = in ? fx * nx + cx : 0.0, v0 = in ? fy * ny + cy : 0.0;
    double cu = floor(u0), cv = floor(v0);
    if (!(cu > -32000.0)) cu = -32000.0; if (cu > 32000.0) cu = 32000.0;
    if (!(cv > -32000.0)) cv = -32000.0; if (cv > 32000.0) cv = 32000.0;
    const_cast<float*>(A.f0x)[o] = (float)(u0 - cu);
    const_cast<float*>(A.f0y)[o] = (float)(v0 - cv);
    const_cast<int*>(A.cell0)[o] = (int)(((unsigned)(int)cv << 16) | ((unsigned)(int)cu & 0xffffu));
}
__global__ __launch_bounds__(KF_T) void k_fill_slot(EdsArrays A, int slot, int N, double fx, double fy, double cx, double cy,
                                                    const double* __restrict__ coord, const double* __restrict__ grad,
                                                    const double* __restrict__ idp, const double* __restrict__ w) {
    d_fill_slot(A, slot, N, fx, fy, cx, cy, coord, grad, idp, w);
}
// slot first + blockIdx.y of a chunk, K (4 doubles per slot) and the counts from device memory.  A slot is filled only where the single call
// would have filled it: a tree built here (flag 0), at least one candidate, 1 .. Nmax points kept; every other slot stays as it is.
__global__ __launch_bounds__(KF_T) void k_fill_slot_b(EdsArrays A, int first, int Nmax, const double* __restrict__ K, const int* __restrict__ summary,
                                                      size_t npx, const double* __restrict__ coord, const double* __restrict__ grad,
                                                      const double* __restrict__ idp, const double* __restrict__ w) {
    const size_t y = blockIdx.y;
    const int ncand = summary[4 * y], N = summary[4 * y + 1], flag = summary[4 * y + 3];
    if (flag != 0 || ncand < 1 || N < 1 || N > Nmax) return;
    d_fill_slot(A, first + (int)y, N, K[4 * y], K[4 * y + 1], K[4 * y + 2], K[4 * y + 3], coord + 2 * y * npx, grad + 2 * y * npx, idp + y * npx, w + y * npx);
}

}  // namespace
