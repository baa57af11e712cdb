// The order-statistic primitive of the per-alignment selections (eds_points.hip k_loss_param, eds_depth.hip k_depth_stats): a
// most-significant-digit radix select on order-preserving 64-bit keys, one workgroup of EDS_LP_THREADS per alignment.
#pragma once
#include <hip/hip_runtime.h>

#define EDS_LP_THREADS 256

namespace edssel {

// order-preserving map double -> uint64 (and back): a radix select on these keys returns exactly the order statistic a sort would
__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double val_of(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// The k-th smallest (0-based) of the N keys `key(i)`: most-significant-digit radix select, 8 bits per pass — histogram of the
// candidates' digit in LDS, a wavefront scan picks the bin holding rank k, the candidates narrow to that bin.  Stops as soon as
// one candidate is left (2 000 keys: after 2-3 passes) and fetches it.  O(N) per pass against the O(N log^2 N) compare-exchanges
// and 66 workgroup barriers of the bitonic sort it replaces (60 us per alignment; this: ~5 us), no key buffer in LDS, any N.
template <class KeyFn>
__device__ unsigned long long radix_select(KeyFn key, int N, int k, int tid, int* hist, unsigned long long* s_sel, int* s_cnt) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += EDS_LP_THREADS) hist[i] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < N; i0 += EDS_LP_THREADS) {           // (uniform trip count: the wavefront votes below need every lane)
            const int i = i0 + tid;
            int digit = -1;                                         // -1: not a candidate
            if (i < N) {
                const unsigned long long q = key(i);
                if ((q & mask) == prefix) digit = (int)((q >> shift) & 255ull);
            }
            // residuals of one alignment share sign / exponent digits: a plain LDS atomic per lane would serialise on one or two
            // bins.  Up to four rounds of "the first pending lane's digit, counted by a ballot, added once"; what is still pending
            // after that is spread over many bins and goes in lane by lane.
#pragma unroll 1
            for (int round = 0; round < 4; ++round) {
                const unsigned long long pending = __ballot(digit >= 0);
                if (pending == 0ull) break;
                const int d = __shfl(digit, __ffsll((long long)pending) - 1, 64);
                const unsigned long long same = __ballot(digit == d);
                if ((tid & 63) == __ffsll((long long)same) - 1) atomicAdd(&hist[d], __popcll(same));
                if (digit == d) digit = -1;
            }
            if (digit >= 0) atomicAdd(&hist[digit], 1);
        }
        __syncthreads();
        if (tid < 64) {                 // bins 4 tid .. 4 tid + 3
            const int c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const int mine = c0 + c1 + c2 + c3;
            int incl = mine;
            for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (tid >= off) incl += v; }
            const int excl = incl - mine;
            if (excl <= k && k < incl) {        // exactly one lane
                int r = k - excl, bin = 4 * tid, cnt = c0;
                if (r >= c0) { r -= c0; bin = 4 * tid + 1; cnt = c1;
                    if (r >= c1) { r -= c1; bin = 4 * tid + 2; cnt = c2;
                        if (r >= c2) { r -= c2; bin = 4 * tid + 3; cnt = c3; } } }
                s_sel[0] = prefix | ((unsigned long long)bin << shift);
                s_cnt[0] = r; s_cnt[1] = cnt;
            }
        }
        __syncthreads();
        prefix = s_sel[0]; mask |= 0xffull << shift;
        k = s_cnt[0];
        const int cnt = s_cnt[1];
        __syncthreads();
        if (cnt == 1 && shift > 0) {    // one candidate left: fetch it
            for (int i = tid; i < N; i += EDS_LP_THREADS) {
                const unsigned long long q = key(i);
                if ((q & mask) == prefix) s_sel[0] = q;
            }
            __syncthreads();
            prefix = s_sel[0];
            __syncthreads();
            return prefix;
        }
    }
    return prefix;
}

}  // namespace edssel
