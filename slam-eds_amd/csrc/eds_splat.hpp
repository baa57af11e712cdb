// The sparse bilinear splat and its 3 x 3 blur, shared by the KLT window kernel (eds_klt.hip) and the epiline model image
// (eds_epiline.hip): drawValuesPoints (reference src/utils/Utils.cpp:124-193) without a dense image.  k_klt_bin sorts one key per
// point, (y0, x0, i) = the top-left corner of its bilinear footprint and its index; a pixel then sums the four runs of keys whose
// footprint has a corner on it, merged in ascending i, so every pixel adds its contributions in the reference's order.
//
// fp64 without FMA contraction: the arithmetic below switches contraction off itself where the compiler honours the pragma, and the
// translation units that include this header are compiled with -ffp-contract=off as well (Makefile).  Plain C++ can include it
// (tests/cpp/splat_check.cpp); only the wavefront reductions need hipcc.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/eds_hip_epiline.h"

#if defined(__HIPCC__)
#define EDS_SPLAT_FN __host__ __device__ __forceinline__
#else
#define EDS_SPLAT_FN inline
#endif
#if defined(__clang__)
#define EDS_SPLAT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EDS_SPLAT_NO_CONTRACT
#endif

namespace edssplat {

// the key: row y0, key column x0 (16 bits each, biased by the caller so that neither is negative), point index i
EDS_SPLAT_FN uint64_t splat_key(int y0, int x0, int i) { return ((uint64_t)y0 << 48) | ((uint64_t)x0 << 32) | (uint64_t)i; }
EDS_SPLAT_FN int key_y0(uint64_t k) { return (int)(k >> 48); }
EDS_SPLAT_FN int key_x0(uint64_t k) { return (int)((k >> 32) & 0xffffu); }
EDS_SPLAT_FN unsigned key_i(uint64_t k) { return (unsigned)(k & 0xffffffffu); }

// first q in [lo, hi) whose key has x0 >= xv (the keys of one row ascend in x0)
EDS_SPLAT_FN int lower_x(const uint64_t* K, int lo, int hi, int xv) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key_x0(K[mid]) < xv) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// cv::borderInterpolate(p, len, type) for REPLICATE, REFLECT and REFLECT_101, repeated while p is outside (a window wider than the image)
EDS_SPLAT_FN int border_map(int p, int len, int type) {
    if ((unsigned)p < (unsigned)len) return p;
    if (type == EDS_EPI_BORDER_REPLICATE) return p < 0 ? 0 : len - 1;
    if (len == 1) return 0;
    const int delta = type == EDS_EPI_BORDER_REFLECT_101 ? 1 : 0;
    do {
        if (p < 0) p = -p - 1 + delta;
        else p = len - 1 - (p - len) - delta;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}
EDS_SPLAT_FN int reflect101(int p, int len) { return border_map(p, len, EDS_EPI_BORDER_REFLECT_101); }

// One key row [q, hi), q its first key with key column >= kx (the caller's search): g[0] = the run with key column kx, g[1] = kx + 1
EDS_SPLAT_FN void splat_runs(const uint64_t* K, int q, int hi, int kx, int (*g)[2]) {
    g[0][0] = q;
    while (q < hi && key_x0(K[q]) == kx) ++q;
    g[0][1] = q; g[1][0] = q;
    while (q < hi && key_x0(K[q]) == kx + 1) ++q;
    g[1][1] = q;
}

// The splat values of pixel (py, px): s[v] = sum of w V[v][m] over the points m of four runs, g[0], g[1] from splat_runs of row
// y0 = py - 1 at x0 = px - 1, g[2], g[3] of row y0 = py.  Their footprint corner on the pixel is (y1, x1) [weight wd], (y1, x0) [wb],
// (y0, x1) [wc], (y0, x0) [wa]; each run ascends in m and the four are merged, so the sum runs in point order.  C: the points'
// coordinates [..][2].  Corners outside the image carry weight 0 in the reference and land on a clipped pixel: adding +-0 to a sum that
// starts at +0 changes nothing, so no key exists for them.
template <int NV, typename T>
EDS_SPLAT_FN void splat_merge(const uint64_t* K, int (&g)[4][2], const double* C, const T* const* V, double (&s)[NV]) {
    EDS_SPLAT_NO_CONTRACT
    for (int v = 0; v < NV; ++v) s[v] = 0.0;
    while (true) {
        unsigned m = UINT_MAX;
        int which = -1;
        for (int c = 0; c < 4; ++c)
            if (g[c][0] < g[c][1]) {
                const unsigned ic = key_i(K[g[c][0]]);
                if (ic < m) { m = ic; which = c; }
            }
        if (which < 0) break;
        ++g[which][0];
        const double xj = C[2 * m], yj = C[2 * m + 1];
        const double x0 = floor(xj), y0 = floor(yj), x1 = x0 + 1.0, y1 = y0 + 1.0;
        double w;
        if (which == 0) w = (xj - x0) * (yj - y0);            // wd at (y1, x1)
        else if (which == 1) w = (x1 - xj) * (yj - y0);       // wb at (y1, x0)
        else if (which == 2) w = (xj - x0) * (y1 - yj);       // wc at (y0, x1)
        else w = (x1 - xj) * (y1 - yj);                       // wa at (y0, x0)
        for (int v = 0; v < NV; ++v) s[v] = s[v] + w * (double)V[v][m];
    }
}

// cv::getGaussianKernel(3, 0.5, CV_64F): [k0, k1, k0] = [t, 1, t] / (1 + 2t)
EDS_SPLAT_FN void gauss3_sigma_half(double& k0, double& k1) {
    EDS_SPLAT_NO_CONTRACT
    const double t = std::exp(-0.5 / (0.5 * 0.5));
    k0 = t / (1.0 + 2.0 * t); k1 = 1.0 / (1.0 + 2.0 * t);
}

// cv::GaussianBlur 3 x 3 at image pixel (oy, ox): rows first, then columns, each k0 a + k1 b + k2 c on reflect-101 neighbours.  box: the
// splat values of image columns bx0 .. bx0 + bw - 1 from row by0 on, which hold the pixel and its neighbours
EDS_SPLAT_FN double blur3_at(const double* box, int bw, int bx0, int by0, int ox, int oy, int W, int H, double k0, double k1, double k2) {
    EDS_SPLAT_NO_CONTRACT
    const int xl = reflect101(ox - 1, W) - bx0, xc = ox - bx0, xr = reflect101(ox + 1, W) - bx0;
    const int yu = reflect101(oy - 1, H) - by0, yc = oy - by0, yd = reflect101(oy + 1, H) - by0;
    const double ru = k0 * box[yu * bw + xl] + k1 * box[yu * bw + xc] + k2 * box[yu * bw + xr];
    const double rc = k0 * box[yc * bw + xl] + k1 * box[yc * bw + xc] + k2 * box[yc * bw + xr];
    const double rd = k0 * box[yd * bw + xl] + k1 * box[yd * bw + xc] + k2 * box[yd * bw + xr];
    return k0 * ru + k1 * rc + k2 * rd;
}

#if defined(__HIPCC__)
__device__ __forceinline__ double wave_sum(double v) {      // xor butterfly: every lane ends with the same, fixed-order total
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}
#endif

}  // namespace edssplat
