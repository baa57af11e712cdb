// What the DSO-side modules (eds_coarse, eds_window, eds_winsolve, eds_winflag, eds_winedit, eds_immature, eds_activate, eds_pixsel,
// eds_init, eds_inisetup, eds_map, eds_undistort) share, once each: the host/device macro, the finiteness helpers, one pixel of a frame
// level with makeImages' box filter and gradient, getInterpolatedElement's cell and weights, the sum order, and on the device the fold
// inside a wavefront and the stable rank inside a workgroup.  Range checks stay with the callers: they differ per reference function.
// Every translation unit that includes this is built without contraction into FMAs.  Plain C++17 outside hipcc.
//
// THE SUM ORDER.  A sum over the entries of a list is taken by LANES = 512 lanes.  Lane t adds, starting from 0.0 and in fp64, the terms
// of entries t, t + 512, t + 1024, ... in that order (an entry that contributes nothing adds nothing).  Inside every 64 consecutive lanes
// the partials are folded by p[t] += p[t + s] for (t mod 64) < s, s = 32, 16, 8, 4, 2, 1; the eight group totals are added left to right.
// reduce_lanes() is that fold on the host; the device does the same with wave_fold() and add8() over eight LDS words.  Counts are integers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

// the same two definitions as eds_math.hpp's, token for token: a translation unit may include both
#if defined(__HIPCC__)
#define EDS_HD __host__ __device__ inline
#else
#define EDS_HD inline
#endif
#if defined(__clang__)
#define EDS_UNROLL _Pragma("unroll")             /* the device needs constant indices: a local array must stay in registers */
#else
#define EDS_UNROLL
#endif

namespace edsdso {

constexpr int LANES = 512;
constexpr int WAVE = 64;
constexpr int GROUPS = LANES / WAVE;

EDS_HD bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }          // false for NaN and +-inf
EDS_HD bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }
EDS_HD float nan_f() { return __builtin_nanf(""); }
EDS_HD double nan_d() { return __builtin_nan(""); }

struct NoSync { EDS_HD void operator()() const {} };            // the barrier of a serial walk

// ---- makeImages (HessianBlocks.cpp:139-202) -----------------------------------------------------------------------------------------
struct alignas(16) Px { float c, dx, dy, pad; };                // one pixel of a frame level

EDS_HD float down_at(const Px* lm, int wlm1, int x, int y) {
    const int b = 2 * x + 2 * y * wlm1;
    return 0.25f * (((lm[b].c + lm[b + 1].c) + lm[b + wlm1].c) + lm[b + 1 + wlm1].c);
}

// the gradient rule of every layout: zero on the first and the last row, else the central difference with a non-finite one set to zero
EDS_HD bool border_row(int w, int h, int i) { return i < w || i >= w * (h - 1); }
EDS_HD float half_diff(float hi, float lo) {
    const float d = 0.5f * (hi - lo);
    return finite_f(d) ? d : 0.0f;
}

EDS_HD void gradient_at(const Px* p, int w, int h, int i, float* dx_out, float* dy_out) {
    *dx_out = 0.0f; *dy_out = 0.0f;
    if (border_row(w, h, i)) return;
    *dx_out = half_diff(p[i + 1].c, p[i - 1].c);
    *dy_out = half_diff(p[i + w].c, p[i - w].c);
}

// pixel i of a level w wide before its gradient: from the dense image (lm == NULL, level 0) or from the level below, wlm1 wide
EDS_HD Px level_pixel(const float* img, const Px* lm, int wlm1, int w, int i) {
    Px o;
    o.c = lm ? down_at(lm, wlm1, i % w, i / w) : img[i];
    o.dx = 0.0f; o.dy = 0.0f; o.pad = 0.0f;
    return o;
}

// ---- getInterpolatedElement (globalFuncs.h:78-133) ----------------------------------------------------------------------------------
// the cell of a sample and its four weights; w00 is ((1 - dx) - dy) + dxdy
struct Bilin { int ix, iy; float w00, w10, w01, w11; };

EDS_HD Bilin bilin(float x, float y) {
    Bilin b;
    b.ix = (int)x; b.iy = (int)y;
    const float dx = x - b.ix, dy = y - b.iy, dxdy = dx * dy;
    b.w11 = dxdy; b.w01 = dy - dxdy; b.w10 = dx - dxdy; b.w00 = 1 - dx - dy + dxdy;
    return b;
}

// v11 is the cell's (ix + 1, iy + 1), v01 (ix, iy + 1), v10 (ix + 1, iy), v00 (ix, iy): summed left to right
EDS_HD float mix(const Bilin& w, float v11, float v01, float v10, float v00) { return w.w11 * v11 + w.w01 * v01 + w.w10 * v10 + w.w00 * v00; }

// ---- the sum order ------------------------------------------------------------------------------------------------------------------
EDS_HD double add8(const double* p) { return ((((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5]) + p[6]) + p[7]; }

#if defined(__HIPCC__)
// the fold inside 64 lanes: lane 0 of the wavefront holds the total
__device__ inline double wave_fold(double v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    return v;
}
__device__ inline int wave_fold_i(int v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    return v;
}

// The stable rank of this lane's kept element among the kept ones of a workgroup of T threads, in thread order, and their number: the
// wavefronts before its own (s_wave: T / 64 words of LDS) plus the set bits of the ballot below its lane.  Every thread of the workgroup
// calls it; the second barrier lets a sweep call it again with the same s_wave.
template <int T>
__device__ __forceinline__ int block_rank(bool keep, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) { const int n = s_wave[w]; before += w < wave ? n : 0; sum += n; }
    __syncthreads();
    *total = sum;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// The prologue of a grid-wide compaction whose first kernel left every workgroup's count in block_cnt[]: the sum of the counts before
// this workgroup, in every thread.  s_wave as block_rank's, and free for it afterwards.
template <int T>
__device__ __forceinline__ int blocks_before(const int32_t* __restrict__ block_cnt, int* s_wave) {
    int v = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += T) v += block_cnt[b];
    v = wave_fold_i(v);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    int sum = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) sum += s_wave[w];
    __syncthreads();
    return sum;
}
#endif

// ---- the host's side: the fold in the device's order, and a frame's levels ------------------------------------------------------------
inline double reduce_lanes(double* p) {
    for (int g = 0; g < GROUPS; ++g)
        for (int s = WAVE / 2; s >= 1; s >>= 1)
            for (int t = 0; t < s; ++t) p[g * WAVE + t] += p[g * WAVE + t + s];
    double r = p[0];
    for (int g = 1; g < GROUPS; ++g) r += p[g * WAVE];
    return r;
}

// `levels` levels of makeImages on the host: level l is (w >> l) x (h >> l) at px[l], its colours first, then its gradients
inline void make_levels(const float* image, int64_t row_stride, int w, int h, int levels, Px* const* px) {
    for (int l = 0; l < levels; ++l) {
        const int wl = w >> l, hl = h >> l;
        Px* p = px[l];
        for (int y = 0; y < hl; ++y)
            for (int x = 0; x < wl; ++x)
                p[x + y * wl] = l == 0 ? level_pixel(image + (int64_t)y * row_stride, nullptr, 0, wl, x) : level_pixel(nullptr, px[l - 1], w >> (l - 1), wl, x + y * wl);
        for (int i = 0; i < wl * hl; ++i) gradient_at(p, wl, hl, i, &p[i].dx, &p[i].dy);
    }
}

}  // namespace edsdso

// the fold was edsct's before it moved here; the window's and the solver's g++ harnesses name it so without the coarse tracker's header
namespace edsct { using edsdso::reduce_lanes; }
