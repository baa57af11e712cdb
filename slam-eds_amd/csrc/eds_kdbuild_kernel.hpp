// k_kd_build, the device build of the depth k-d tree (eds_kdbuild.hpp states its steps), and its launch: shared by the keyframe switch of an
// eds_trk (eds_kfswitch.hip) and the depth-seeded immature points of an eds_imm (eds_immdepth.hip).  One workgroup per map: the points
// (fp64 pairs, 16-byte LDS accesses), three 16-bit index lists, a scan array and the side marks in LDS, 27 bytes per point, 4 096 points
// in 108 KiB.  Two bitonic sorts (by x, by y; equal values by index) run side by side; then, level by level, the node of every
// sub-range is the middle of its axis-sorted list, and the other axis' list is partitioned stably by side with wave64 ballots and
// popcounts.  It writes the map in tree order (txy, tidp, the permutation) and one flag per map: 0 built, 1 ambiguous or not finite (the
// build stops at the level that shows it), 2 more points than the launch holds.  Internal linkage: each translation unit gets its own
// copy of the same code, and reserves the kernel's LDS itself (kd_build_reserve).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "eds_device_owner.hpp"
#include "eds_kdbuild.hpp"

namespace {

// One workgroup (blockDim.x a multiple of 64, <= edskdb::THREADS) per map b = blockIdx.x; M2: a power of two >= 64, the points the
// dynamic LDS (edskdb::lds_bytes(M2)) holds.  xy / idp: the map at b * in_stride; perm / txy / tidp: its tree order at b * out_stride.
__global__ __launch_bounds__(edskdb::THREADS) void k_kd_build(const double* __restrict__ xy, const double* __restrict__ idp, size_t in_stride,
                                                              const int* __restrict__ map_n, int M2, size_t out_stride, int* __restrict__ perm,
                                                              double* __restrict__ txy, double* __restrict__ tidp, int* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kd_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = T >> 6;
    const int m = map_n[b];
    if (m < 1) { if (tid == 0) flag[b] = 0; return; }
    if (m > M2) { if (tid == 0) flag[b] = 2; return; }
    double2* sxy = reinterpret_cast<double2*>(kd_lds);
    unsigned* scan = reinterpret_cast<unsigned*>(kd_lds + (size_t)16 * M2);
    unsigned short* lists = reinterpret_cast<unsigned short*>(kd_lds + (size_t)20 * M2);
    unsigned char* side = kd_lds + (size_t)26 * M2;
    unsigned* s_wave = reinterpret_cast<unsigned*>(kd_lds + (size_t)27 * M2);       // [16]
    int* s_amb = reinterpret_cast<int*>(s_wave + 16);
    const double* gxy = xy + 2 * (size_t)b * in_stride;
    if (tid == 0) *s_amb = 0;
    __syncthreads();
    int P2 = 64;                                  // the sorts' size: the power of two that holds m
    while (P2 < m) P2 <<= 1;
    bool bad = false;
    for (int i = tid; i < P2; i += T) {
        const bool in = i < m;
        if (in) {
            const double x = gxy[2 * (size_t)i], y = gxy[2 * (size_t)i + 1];
            sxy[i] = make_double2(x, y);
            bad = bad || !edskdb::finite_xy(x, y);
        }
        lists[i] = lists[M2 + i] = in ? (unsigned short)i : (unsigned short)0xffff;       // padding sorts behind every point
    }
    if (bad) *s_amb = 1;
    __syncthreads();
    if (*s_amb) { if (tid == 0) flag[b] = 1; return; }
    // both index lists sorted at once: list 0 by x, list 1 by y (bitonic network; edskdb::key_before)
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & k) == 0;
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        unsigned short* L = lists + (size_t)a * M2;
                        const int ia = L[i], ib = L[ixj];
                        bool b_first;                 // the element at ixj belongs in front of the one at i
                        if (ib >= m) b_first = false;
                        else if (ia >= m) b_first = true;
                        else {
                            const double2 pa = sxy[ia], pb = sxy[ib];
                            b_first = edskdb::key_before(a ? pb.y : pb.x, ib, a ? pa.y : pa.x, ia);
                        }
                        if (b_first == up) { L[i] = (unsigned short)ib; L[ixj] = (unsigned short)ia; }
                    }
                }
            }
            __syncthreads();
        }
    }
    int cur0 = 0, cur1 = 1, spare = 2;
    const int D = edskdb::levels(m);
    for (int level = 0; level < D; ++level) {
        const int a = level & 1;
        const unsigned short* A = lists + (size_t)(a ? cur1 : cur0) * M2;
        const unsigned short* O = lists + (size_t)(a ? cur0 : cur1) * M2;
        unsigned short* On = lists + (size_t)spare * M2;
        // the sides of every sub-range, and the rule at its node
        for (int p = tid; p < m; p += T) {
            int lo, hi;
            if (!edskdb::segment_of(m, level, p, &lo, &hi)) continue;
            const int mid = edskdb::node_of(lo, hi);
            side[A[p]] = p < mid ? 0 : (p == mid ? 1 : 2);
            if (p == mid) {
                const double2 c = sxy[A[mid]];
                const double kc = a ? c.y : c.x;
                bool amb = false;
                if (mid > lo) { const double2 q = sxy[A[mid - 1]]; amb = amb || (a ? q.y : q.x) == kc; }
                if (mid + 1 < hi) { const double2 q = sxy[A[mid + 1]]; amb = amb || (a ? q.y : q.x) == kc; }
                if (amb) *s_amb = 1;
            }
        }
        __syncthreads();
        if (*s_amb) { if (tid == 0) flag[b] = 1; return; }
        // exclusive counts of left marks (low 16 bits) and right marks (high 16 bits) along the other list
        unsigned run = 0;
        for (int c0 = 0; c0 < m; c0 += T) {
            const int p = c0 + tid;
            const int s = p < m ? side[O[p]] : 1;
            const unsigned long long bl = __ballot(s == 0), br = __ballot(s == 2);
            if (lane == 0) s_wave[wave] = (unsigned)__popcll(bl) | ((unsigned)__popcll(br) << 16);
            __syncthreads();
            unsigned before = 0, total = 0;
            for (int w = 0; w < nwave; ++w) { const unsigned v = s_wave[w]; before += w < wave ? v : 0u; total += v; }
            const unsigned long long lt = (1ull << lane) - 1ull;
            if (p < m) scan[p] = run + before + ((unsigned)__popcll(bl & lt) | ((unsigned)__popcll(br & lt) << 16));
            run += total;
            __syncthreads();
        }
        // stable partition of every sub-range of the other list: left | node | right
        for (int p = tid; p < m; p += T) {
            int lo, hi;
            const unsigned short i = O[p];
            if (!edskdb::segment_of(m, level, p, &lo, &hi)) { On[p] = i; continue; }
            const int mid = edskdb::node_of(lo, hi), s = side[i];
            const unsigned d = scan[p] - scan[lo];
            On[s == 0 ? lo + (int)(d & 0xffffu) : (s == 1 ? mid : mid + 1 + (int)(d >> 16))] = i;
        }
        __syncthreads();
        const int o = a ? cur0 : cur1;
        if (a) cur0 = spare; else cur1 = spare;
        spare = o;
    }
    const unsigned short* L = lists + (size_t)cur0 * M2;
    const size_t ob = (size_t)b * out_stride;
    for (int p = tid; p < m; p += T) {
        const int i = L[p];
        perm[ob + p] = i;
        if (txy) { const double2 c = sxy[i]; txy[2 * (ob + p)] = c.x; txy[2 * (ob + p) + 1] = c.y; }
        if (tidp) tidp[ob + p] = idp[(size_t)b * in_stride + i];
    }
    if (tid == 0) flag[b] = 0;
}

// the right of k_kd_build to its LDS, once per translation unit and device context
inline int kd_build_reserve() {
    EDS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_kd_build), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)edskdb::lds_bytes(edskdb::CAPACITY)));
    return EDS_OK;
}

// cn maps queued into st, nothing waited for: map b of d_mn[b] points at b * in_stride of d_xy / d_idp (d_idp, d_txy, d_tidp may be NULL),
// its tree order at b * out_stride; max_m: the largest d_mn, which sizes the workgroup and its LDS
inline int kd_build_launch(hipStream_t st, int cn, const double* d_xy, const double* d_idp, size_t in_stride, const int* d_mn, int max_m,
                           size_t out_stride, int* d_perm, double* d_txy, double* d_tidp, int* d_flag) {
    const int M2 = edskdb::pow2_at_least(std::min(std::max(max_m, 1), edskdb::CAPACITY));
    const int T = std::min(M2, edskdb::THREADS);
    hipLaunchKernelGGL(k_kd_build, dim3(cn), dim3(T), edskdb::lds_bytes(M2), st, d_xy, d_idp, in_stride, d_mn, M2, out_stride, d_perm, d_txy, d_tidp,
                       d_flag);
    EDS_HIP_TRY(hipGetLastError());
    return EDS_OK;
}

}  // namespace
