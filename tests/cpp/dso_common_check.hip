// The device helpers of slam-eds_amd/csrc/eds_dso_common.hpp against serial restatements, a stand-alone program (tests/test_dso_common.py
// builds and runs it once): block_rank<T> in a sweeping workgroup of T = 256, 512 and 1024 threads, the two-kernel grid compaction
// (__syncthreads_count, blocks_before, block_rank<256>), wave_fold + add8 against reduce_lanes bit for bit, and wave_fold_i.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>

#include "eds_dso_common.hpp"

#define CHECK_HIP(expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            std::printf("%s: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__);               \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

namespace {

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// one workgroup sweeps n elements T at a time: rank[i] is the place of kept element i among the kept ones, -1 for the others
template <int T>
__global__ void __launch_bounds__(T) k_sweep(const uint8_t* __restrict__ keep, int n, int32_t* __restrict__ rank, int32_t* __restrict__ total_out) {
    __shared__ int s_wave[T / 64];
    int run = 0;
    for (int c0 = 0; c0 < n; c0 += T) {
        const int i = c0 + (int)threadIdx.x;
        const bool k = i < n && keep[i] != 0;
        int total;
        const int r = edsdso::block_rank<T>(k, s_wave, &total);
        if (i < n) rank[i] = k ? run + r : -1;
        run += total;
    }
    if (threadIdx.x == 0) *total_out = run;
}

__global__ void __launch_bounds__(256) k_count(const uint8_t* __restrict__ keep, int n, int32_t* __restrict__ block_cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int c = __syncthreads_count(i < n && keep[i] != 0);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = c;
}

// the kept indices in order: list[0 .. *total_out)
__global__ void __launch_bounds__(256) k_compact(const uint8_t* __restrict__ keep, int n, const int32_t* __restrict__ block_cnt, int32_t* __restrict__ list,
                                                 int32_t* __restrict__ total_out) {
    __shared__ int s_wave[256 / 64];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int base = edsdso::blocks_before<256>(block_cnt, s_wave);
    const bool k = i < n && keep[i] != 0;
    int total;
    const int r = edsdso::block_rank<256>(k, s_wave, &total);
    if (k) list[base + r] = i;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = base + total;
}

// THE SUM ORDER over m entries, and the integer fold of every wavefront's lane values
__global__ void __launch_bounds__(edsdso::LANES) k_fold(const double* __restrict__ x, int m, double* __restrict__ sum, const int32_t* __restrict__ iv,
                                                       int32_t* __restrict__ isum) {
    __shared__ double part[edsdso::GROUPS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v = 0.0;
    for (int i = threadIdx.x; i < m; i += edsdso::LANES) v += x[i];
    v = edsdso::wave_fold(v);
    const int c = edsdso::wave_fold_i(iv[threadIdx.x]);
    if (lane == 0) { part[wave] = v; isum[wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0) *sum = edsdso::add8(part);
}

std::vector<uint8_t> pattern(int n, int kind, uint64_t seed) {
    std::vector<uint8_t> k((size_t)n);
    for (int i = 0; i < n; ++i) k[i] = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? (i % 3 == 0) : (uint8_t)(splitmix(seed) & 1u);
    return k;
}

template <int T>
int check_sweep(uint8_t* d_keep, int32_t* d_rank, int32_t* d_total, int* failures) {
    const int sizes[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1};
    for (int n : sizes)
        for (int kind = 0; kind < 4; ++kind) {
            const std::vector<uint8_t> keep = pattern(n, kind, 1000u * T + 10u * n + kind);
            std::vector<int32_t> want((size_t)n), got((size_t)n, -2);
            int run = 0;
            for (int i = 0; i < n; ++i) want[i] = keep[i] ? run++ : -1;
            int32_t total = -1;
            if (n) CHECK_HIP(hipMemcpy(d_keep, keep.data(), (size_t)n, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_sweep<T>, dim3(1), dim3(T), 0, 0, d_keep, n, d_rank, d_total);
            CHECK_HIP(hipGetLastError());
            CHECK_HIP(hipDeviceSynchronize());
            if (n) CHECK_HIP(hipMemcpy(got.data(), d_rank, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
            CHECK_HIP(hipMemcpy(&total, d_total, sizeof(total), hipMemcpyDeviceToHost));
            if (total != run || got != want) {
                std::printf("block_rank<%d>: n = %d, pattern %d: total %d (want %d)%s\n", T, n, kind, total, run, got != want ? ", ranks differ" : "");
                ++*failures;
            }
        }
    return 0;
}

}  // namespace

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::printf("no device\n"); return 2; }
    constexpr int MAX_N = 2 * 1024 + 1;
    uint8_t* d_keep = nullptr;
    int32_t *d_rank = nullptr, *d_total = nullptr, *d_cnt = nullptr, *d_iv = nullptr, *d_isum = nullptr;
    double *d_x = nullptr, *d_sum = nullptr;
    CHECK_HIP(hipMalloc(&d_keep, MAX_N));
    CHECK_HIP(hipMalloc(&d_rank, MAX_N * sizeof(int32_t)));
    CHECK_HIP(hipMalloc(&d_total, sizeof(int32_t)));
    int failures = 0;
    if (int rc = check_sweep<256>(d_keep, d_rank, d_total, &failures)) return rc;
    if (int rc = check_sweep<512>(d_keep, d_rank, d_total, &failures)) return rc;
    if (int rc = check_sweep<1024>(d_keep, d_rank, d_total, &failures)) return rc;

    // the grid-wide compaction over four workgroups, the last of one element
    {
        constexpr int n = 3 * 256 + 1, nb = (n + 255) / 256;
        CHECK_HIP(hipMalloc(&d_cnt, nb * sizeof(int32_t)));
        for (int kind = 0; kind < 4; ++kind) {
            const std::vector<uint8_t> keep = pattern(n, kind, 77u + kind);
            std::vector<int32_t> want, got((size_t)n, -2);
            for (int i = 0; i < n; ++i) if (keep[i]) want.push_back(i);
            int32_t total = -1;
            CHECK_HIP(hipMemcpy(d_keep, keep.data(), (size_t)n, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_count, dim3(nb), dim3(256), 0, 0, d_keep, n, d_cnt);
            hipLaunchKernelGGL(k_compact, dim3(nb), dim3(256), 0, 0, d_keep, n, d_cnt, d_rank, d_total);
            CHECK_HIP(hipGetLastError());
            CHECK_HIP(hipDeviceSynchronize());
            CHECK_HIP(hipMemcpy(got.data(), d_rank, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
            CHECK_HIP(hipMemcpy(&total, d_total, sizeof(total), hipMemcpyDeviceToHost));
            got.resize(total >= 0 && total <= n ? (size_t)total : 0);
            if (total != (int)want.size() || got != want) {
                std::printf("grid compaction: pattern %d: total %d (want %d)%s\n", kind, total, (int)want.size(), got != want ? ", lists differ" : "");
                ++failures;
            }
        }
    }

    // wave_fold + add8 against reduce_lanes bit for bit on magnitudes 2^-30 .. 2^30 (the order matters), and wave_fold_i
    {
        constexpr int m = 3 * edsdso::LANES + 17;
        uint64_t seed = 2024;
        std::vector<double> x((size_t)m);
        for (int i = 0; i < m; ++i) {
            const uint64_t r = splitmix(seed);
            const double frac = 1.0 + (double)(r >> 12) / 4503599627370496.0;                   // [1, 2)
            const int e = (int)(splitmix(seed) % 61u) - 30;
            x[i] = ((r & 1u) ? -frac : frac) * std::ldexp(1.0, e);
        }
        std::vector<int32_t> iv((size_t)edsdso::LANES), isum((size_t)edsdso::GROUPS, -1), iwant((size_t)edsdso::GROUPS, 0);
        for (int t = 0; t < edsdso::LANES; ++t) { iv[t] = (int32_t)(splitmix(seed) % 2001u) - 1000; iwant[t / edsdso::WAVE] += iv[t]; }
        double part[edsdso::LANES], plain = 0.0, got = 0.0;
        for (int t = 0; t < edsdso::LANES; ++t) part[t] = 0.0;
        for (int i = 0; i < m; ++i) { part[i % edsdso::LANES] += x[i]; plain += x[i]; }
        const double want = edsdso::reduce_lanes(part);
        CHECK_HIP(hipMalloc(&d_x, m * sizeof(double)));
        CHECK_HIP(hipMalloc(&d_sum, sizeof(double)));
        CHECK_HIP(hipMalloc(&d_iv, edsdso::LANES * sizeof(int32_t)));
        CHECK_HIP(hipMalloc(&d_isum, edsdso::GROUPS * sizeof(int32_t)));
        CHECK_HIP(hipMemcpy(d_x, x.data(), m * sizeof(double), hipMemcpyHostToDevice));
        CHECK_HIP(hipMemcpy(d_iv, iv.data(), edsdso::LANES * sizeof(int32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_fold, dim3(1), dim3(edsdso::LANES), 0, 0, d_x, m, d_sum, d_iv, d_isum);
        CHECK_HIP(hipGetLastError());
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(&got, d_sum, sizeof(got), hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(isum.data(), d_isum, edsdso::GROUPS * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (std::memcmp(&got, &want, sizeof(got)) != 0) { std::printf("wave_fold + add8: %.17g, reduce_lanes %.17g\n", got, want); ++failures; }
        if (plain == want) { std::printf("the data do not tell the sum order from the plain one\n"); ++failures; }
        if (isum != iwant) { std::printf("wave_fold_i differs\n"); ++failures; }
    }
    (void)hipFree(d_keep); (void)hipFree(d_rank); (void)hipFree(d_total); (void)hipFree(d_cnt);
    (void)hipFree(d_x); (void)hipFree(d_sum); (void)hipFree(d_iv); (void)hipFree(d_isum);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("dso_common ok\n");
    return 0;
}
