// include/eds_hip_coarse.h: DSO's coarse image tracker on the device.  The arithmetic is eds_coarse.hpp, shared with the host; this file
// holds the kernels and the C entry points.  Built without contraction into FMAs (csrc/Makefile).
//
// k_ct_track runs the whole of trackNewestCoarse for one try in ONE workgroup of 512 threads (grid = the batch): the threads stride the
// level's list, keep fp64 partials, fold them in eds_dso_common.hpp's order (its wave_fold, then eight LDS words added by its add8), and
// then EVERY thread runs the small solve, SE3::exp and the accept test on the same workgroup-uniform values — one code path with the
// host, nothing to broadcast.  The 45 sums of calcGSSSE are formed only after an accept (and once per level), as the reference forms
// them, by a second pass that recomputes the accepted pose's rows instead of parking them in HBM: the taps are L2-resident and a try
// needs no scratch area.  512 threads leave each lane 256 VGPRs, which the 45 fp64 partials need (see DESIGN §16 for the table).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_coarse.h"
#include "eds_capi_internal.hpp"
#include "eds_coarse.hpp"

using edscapi::blocks;
using edscapi::fail;
using edsct::Geo;
using edsct::Level;
using edsct::Params;
using edsct::Pc;
using edsct::Photo;
using edsdso::Px;
using edsct::Term;
using edsct::TrackOut;
using edsct::Warp;

static_assert(sizeof(Params) == sizeof(eds_ct_params), "edsct::Params is eds_ct_params member for member");
static_assert(sizeof(TrackOut) == sizeof(eds_ct_result), "edsct::TrackOut is eds_ct_result member for member");
static_assert(sizeof(Term) == 16 * sizeof(float) && sizeof(Term) == sizeof(eds_ct_row), "one row is 16 words");
static_assert(edsct::MAX_DECISIONS == EDS_CT_MAX_DECISIONS && edsct::MAX_LEVELS == EDS_CT_MAX_LEVELS, "header constants");

struct eds_ct {
    edscapi::DeviceOwner own;
    int max_points = 0, max_tries = 0;
    Geo geo;
    Params prm;
    Photo ph;
    bool calib_set = false, ref_set = false, new_set = false;
    int32_t pc_n[edsct::MAX_LEVELS] = {0, 0, 0, 0, 0};
    int max_blocks = 0;
    Geo* d_geo = nullptr;
    Px *ref_px = nullptr, *new_px = nullptr;             // [geo.total]
    float *idA = nullptr, *wsA = nullptr, *idB = nullptr, *wsB = nullptr;
    Pc* pc = nullptr;
    int32_t *d_pc_n = nullptr, *block_cnt = nullptr, *first = nullptr, *last = nullptr, *pix = nullptr, *dropped = nullptr;
    float *in_img = nullptr, *in_cp = nullptr, *in_hdif = nullptr, *wgt = nullptr;
    TrackOut* d_out = nullptr;
    double *d_T = nullptr, *d_aff = nullptr, *d_min_res = nullptr, *d_calc = nullptr;    // d_calc: rs[6], H[64], b[8]
    Term* d_rows = nullptr;
};

namespace {

constexpr int TB = 256;

// The scatter into idepth[0] / weightSums[0], equal to the serial loop in input order.  Pass 0: every contribution finds its pixel
// and weight and records, with INTEGER atomics, the smallest and the largest input index that lands on the pixel.  Pass 1: a pixel with
// one contribution (first == last) is written directly as 0 + x; for any other pixel the contribution with the smallest index walks
// the inputs from itself to the largest index and adds those of its pixel in index order.  No float atomic, no dependence on scheduling.
// The walk is O(last - first) per colliding pixel, n^2 / 2 steps at the worst: eds_ct_create caps n at EDS_CT_MAX_POINTS for that reason.
__global__ void __launch_bounds__(TB) k_ct_splat(int pass, int n, const float* __restrict__ cp, const float* __restrict__ hdif, int W, int H,
                                                 int32_t* pix, float* wgt, int32_t* first, int32_t* last, int32_t* dropped, float* idA, float* wsA) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (pass == 0) {
        int p;
        if (!edsct::splat_pixel(cp[3 * i], cp[3 * i + 1], W, H, &p)) {
            pix[i] = -1;
            atomicAdd(dropped, 1);
            return;
        }
        pix[i] = p;
        wgt[i] = edsct::splat_weight(hdif[i]);
        atomicMin(&first[p], i);
        atomicMax(&last[p], i);
        return;
    }
    const int p = pix[i];
    if (p < 0 || first[p] != i) return;
    const int end = last[p];
    float id = 0.0f, ws = 0.0f;
    for (int j = i; j <= end; j += 8) {                 // eight loads in flight per trip (measured at 14 000 inputs: 1.27 -> 1.16 ms)
        int q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = j + k <= end ? pix[j + k] : -1;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (q[k] == p) { id += cp[3 * (j + k) + 2] * wgt[j + k]; ws += wgt[j + k]; }
    }
    idA[p] = id;
    wsA[p] = ws;
}

__global__ void __launch_bounds__(TB) k_ct_levels(float* idA, float* wsA, const Geo* __restrict__ g, int lvl) {
    const Level L = g->l[lvl], M = g->l[lvl - 1];
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= L.w * L.h) return;
    idA[L.off + i] = edsct::level_sum(idA + M.off, M.w, i % L.w, i / L.w);
    wsA[L.off + i] = edsct::level_sum(wsA + M.off, M.w, i % L.w, i / L.w);
}

// dilation (out of place: A is the reference's _bak) and normalisation of one pixel; the workgroup's number of list entries
__global__ void __launch_bounds__(TB) k_ct_dilate(const float* __restrict__ idA, const float* __restrict__ wsA, float* __restrict__ idB,
                                                  float* __restrict__ wsB, const Px* __restrict__ ref, const Geo* __restrict__ g, int lvl,
                                                  int32_t* __restrict__ block_cnt) {
    const Level L = g->l[lvl];
    const int i = blockIdx.x * TB + threadIdx.x;
    int sel = 0;
    if (i < L.w * L.h) {
        float id, ws;
        edsct::dilate_at(idA + L.off, wsA + L.off, L.w, L.h, lvl, i, &id, &ws);
        sel = edsct::normalise_at(i % L.w, i / L.w, L.w, L.h, ref[L.off + i].c, &id, &ws) ? 1 : 0;
        idB[L.off + i] = id;
        wsB[L.off + i] = ws;
    }
    const int c = __syncthreads_count(sel);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = c;
}

// the stable, row-major compaction: a workgroup's base is the sum of the counts before it (blocks_before), a pixel's place in the
// workgroup block_rank's.  An interior pixel is in the list exactly when its idepth is > 0.
__global__ void __launch_bounds__(TB) k_ct_select(const float* __restrict__ idB, const Px* __restrict__ ref, Pc* __restrict__ pc,
                                                  int32_t* __restrict__ pc_n, const int32_t* __restrict__ block_cnt, const Geo* __restrict__ g, int lvl) {
    __shared__ int s_wave[TB / 64];
    const Level L = g->l[lvl];
    const int i = blockIdx.x * TB + threadIdx.x;
    const int x = i % L.w, y = i / L.w;
    const bool sel = i < L.w * L.h && x >= 2 && x < L.w - 2 && y >= 2 && y < L.h - 2 && idB[L.off + i] > 0;     // in flight with blocks_before's loads
    const int base = edsdso::blocks_before<TB>(block_cnt, s_wave);
    int total;
    const int rank = edsdso::block_rank<TB>(sel, s_wave, &total);
    if (sel) {
        Pc e;
        e.u = (float)x; e.v = (float)y; e.idepth = idB[L.off + i]; e.color = ref[L.off + i].c;
        pc[L.off + base + rank] = e;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) pc_n[lvl] = base + total;
}

// ---- the evaluator of edsct::track on the device --------------------------------------------------------------------------------------
using edsdso::add8;
using edsdso::wave_fold;
using edsdso::wave_fold_i;

// a Warp is the same in every lane: say so, and its 31 words live in scalar registers through the strided loops
__device__ inline Warp uniform_warp(Warp w) {
    static_assert(sizeof(Warp) % 4 == 0, "words");
    int v[sizeof(Warp) / 4];
    __builtin_memcpy(v, &w, sizeof(w));
#pragma unroll
    for (unsigned i = 0; i < sizeof(Warp) / 4; ++i) v[i] = __builtin_amdgcn_readfirstlane(v[i]);
    __builtin_memcpy(&w, v, sizeof(w));
    return w;
}

struct DevEval {
    const Geo* g; Params s; Photo ph;
    const Px* new_px; const Pc* pc; const int32_t* pc_n;
    double* shH; double* shb; double* shS; double* part; double* shP; int* ipart;      // LDS: [64], [8], [45], [45][8], [18], [4][8]
    __device__ const double* H() const { return shH; }
    __device__ const double* b() const { return shb; }
    // thread 0 stores, hess's barriers publish, every thread loads: the next store is at least one res() — two barriers — later
    __device__ void park(const double* R, const double* t, const double* rs) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) shP[i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) shP[9 + i] = t[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) shP[12 + i] = rs[i];
        }
    }
    __device__ void unpark(double* R, double* t, double* rs) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = shP[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = shP[9 + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) rs[i] = shP[12 + i];
    }
    __device__ static int add8i(const int* p) { return p[0] + p[1] + p[2] + p[3] + p[4] + p[5] + p[6] + p[7]; }

    __device__ void res(int lvl, const double* R, const double* t, double a, double bb, float cutoff, double* rs) {
        const Level L = g->l[lvl];
        const Warp w = uniform_warp(edsct::make_warp(L, lvl, s, ph, R, t, a, bb, cutoff));
        const int n = pc_n[lvl], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        double E = 0.0, sT = 0.0, sRT = 0.0;
        int nE = 0, nSat = 0, nFlow = 0;
        for (int i = threadIdx.x; i < n; i += edsct::LANES) {
            const Term o = edsct::point_term(w, new_px + L.off, pc[L.off + i], i);
            if (o.flow) { sT += (double)o.t1; sT += (double)o.t2; sRT += (double)o.rt1; sRT += (double)o.rt2; ++nFlow; }
            if (o.in_e) { E += (double)o.e; ++nE; nSat += 1 - o.warped; }
        }
        E = wave_fold(E); sT = wave_fold(sT); sRT = wave_fold(sRT);
        nE = wave_fold_i(nE); nSat = wave_fold_i(nSat); nFlow = wave_fold_i(nFlow);
        if (lane == 0) {
            part[wave] = E; part[8 + wave] = sT; part[16 + wave] = sRT;
            ipart[wave] = nE; ipart[8 + wave] = nSat; ipart[16 + wave] = nFlow;
        }
        __syncthreads();
        const double Et = add8(part), sTt = add8(part + 8), sRTt = add8(part + 16);
        const int nEt = add8i(ipart), nSatt = add8i(ipart + 8), nFlowt = add8i(ipart + 16);
        __syncthreads();
        edsct::rs_from_sums(Et, nEt, nSatt, sTt, sRTt, nFlowt, rs);
    }

    __device__ void hess(int lvl, const double* R, const double* t, double a, double bb, float cutoff) {
        const Level L = g->l[lvl];
        const Warp w = uniform_warp(edsct::make_warp(L, lvl, s, ph, R, t, a, bb, cutoff));
        const int n = pc_n[lvl], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        double acc[edsct::NUM_SUMS];
#pragma unroll
        for (int q = 0; q < edsct::NUM_SUMS; ++q) acc[q] = 0.0;
        int nW = 0;
        for (int i = threadIdx.x; i < n; i += edsct::LANES) {
            const Term o = edsct::point_term(w, new_px + L.off, pc[L.off + i], i);
            if (!o.warped) continue;
            ++nW;
            float J[9];
            edsct::jacobian(w, o, J);
            int idx = 0;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const float jw = J[r] * o.weight;
#pragma unroll
                for (int c = r; c < 9; ++c) { acc[idx] += (double)(jw * J[c]); ++idx; }
            }
        }
#pragma unroll
        for (int q = 0; q < edsct::NUM_SUMS; ++q) {
            const double v = wave_fold(acc[q]);
            if (lane == 0) part[8 * q + wave] = v;
        }
        nW = wave_fold_i(nW);
        if (lane == 0) ipart[wave] = nW;
        __syncthreads();
        if (threadIdx.x < edsct::NUM_SUMS) shS[threadIdx.x] = add8(part + 8 * threadIdx.x);
        const int nWt = add8i(ipart);
        __syncthreads();
        if (threadIdx.x < 72) {
            const int r = threadIdx.x / 9, c = threadIdx.x % 9;
            const double v = edsct::h_entry(shS, nWt, r, c);
            if (c < 8) shH[8 * r + c] = v; else shb[r] = v;
        }
        __syncthreads();
    }
};

#define EDS_CT_LDS                                                                                            \
    __shared__ double shH[64], shb[8], shS[edsct::NUM_SUMS], part[edsct::NUM_SUMS * 8], shP[18];              \
    __shared__ int ipart[32];                                                                                 \
    DevEval ev;                                                                                               \
    ev.g = g; ev.s = s; ev.ph = ph; ev.new_px = new_px; ev.pc = pc; ev.pc_n = pc_n;                            \
    ev.shH = shH; ev.shb = shb; ev.shS = shS; ev.part = part; ev.shP = shP; ev.ipart = ipart

__global__ void __launch_bounds__(edsct::LANES) k_ct_track(const Geo* __restrict__ g, Params s, Photo ph, const Px* __restrict__ new_px,
                                                          const Pc* __restrict__ pc, const int32_t* __restrict__ pc_n,
                                                          const double* __restrict__ T_in, const double* __restrict__ aff_in, int coarsest,
                                                          const double* __restrict__ min_res, TrackOut* __restrict__ out) {
    EDS_CT_LDS;
    edsct::track(ev, s, ph, T_in + 12 * blockIdx.x, aff_in + 2 * blockIdx.x, coarsest, min_res, out + blockIdx.x, threadIdx.x == 0);
}

// calcRes and calcGSSSE once, by the evaluator k_ct_track runs: out = rs[6], H[64], b[8]
__global__ void __launch_bounds__(edsct::LANES) k_ct_calc(const Geo* __restrict__ g, Params s, Photo ph, const Px* __restrict__ new_px,
                                                         const Pc* __restrict__ pc, const int32_t* __restrict__ pc_n, int lvl,
                                                         const double* __restrict__ T_in, const double* __restrict__ aff_in, float cutoff,
                                                         double* __restrict__ out) {
    EDS_CT_LDS;
    double R[9], t[3], rs[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = T_in[4 * i + j];
        t[i] = T_in[4 * i + 3];
    }
    ev.res(lvl, R, t, aff_in[0], aff_in[1], cutoff, rs);
    ev.hess(lvl, R, t, aff_in[0], aff_in[1], cutoff);
    if (threadIdx.x < 6) out[threadIdx.x] = threadIdx.x == 0 ? rs[0] : threadIdx.x == 1 ? rs[1] : threadIdx.x == 2 ? rs[2] : threadIdx.x == 3 ? rs[3] : threadIdx.x == 4 ? rs[4] : rs[5];
    if (threadIdx.x < 64) out[6 + threadIdx.x] = shH[threadIdx.x];
    if (threadIdx.x < 8) out[70 + threadIdx.x] = shb[threadIdx.x];
}

// the per-point rows of one calcRes, one thread per list entry
__global__ void __launch_bounds__(TB) k_ct_rows(const Geo* __restrict__ g, Params s, Photo ph, const Px* __restrict__ new_px,
                                                const Pc* __restrict__ pc, const int32_t* __restrict__ pc_n, int lvl,
                                                const double* __restrict__ T_in, const double* __restrict__ aff_in, float cutoff, Term* __restrict__ rows) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= pc_n[lvl]) return;
    const Level L = g->l[lvl];
    double R[9], t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * r + j] = T_in[4 * r + j];
        t[r] = T_in[4 * r + 3];
    }
    const Warp w = edsct::make_warp(L, lvl, s, ph, R, t, aff_in[0], aff_in[1], cutoff);
    rows[i] = edsct::point_term(w, new_px + L.off, pc[L.off + i], i);
}

int check_level(const eds_ct* h, int lvl) {
    if (lvl < 0 || lvl >= h->geo.levels) return fail(EDS_ERR_INVALID, "level " + std::to_string(lvl) + " outside 0 .. " + std::to_string(h->geo.levels - 1));
    return EDS_OK;
}

// the checked image into in_img (dense), then every level of `px`; queued, not waited for
int load_frame(eds_ct* h, Px* px, const float* image, int64_t rs, int on_device) {
    const int H = h->geo.H, W = h->geo.W;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edscapi::upload_image(h->own, h->in_img, H, W, image, rs, on_device)) return rc;
    const Level* L = h->geo.l;
    for (int l = 0; l < h->geo.levels; ++l) {
        edscapi::queue_level(h->own.st, l == 0 ? h->in_img : nullptr, l == 0 ? nullptr : px + L[l - 1].off, l == 0 ? 0 : L[l - 1].w, px + L[l].off, L[l].w, L[l].h);
    }
    EDS_HIP_TRY(hipGetLastError());
    return EDS_OK;
}

bool all_finite_d(const double* x, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false;
    return true;
}

int check_ready(const eds_ct* h) {
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_ct: no calibration set");
    if (!h->ref_set) return fail(EDS_ERR_STATE, "eds_ct: no reference frame set");
    if (!h->new_set) return fail(EDS_ERR_STATE, "eds_ct: no new frame set");
    return EDS_OK;
}

}  // namespace

extern "C" {

int eds_ct_abi_version(void) { return EDS_HIP_COARSE_ABI_VERSION; }

void eds_ct_params_default(eds_ct_params* p) {
    if (!p) return;
    const Params d = edsct::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_ct_create(int device, int H, int W, int levels, int max_points, int max_tries, eds_ct** ct) {
    if (!ct) return fail(EDS_ERR_INVALID, "null output");
    *ct = nullptr;
    if (!edsct::shape_valid(H, W, levels))
        return fail(EDS_ERR_INVALID, "levels are 1 .. 5, H and W 8 .. 8192 and divisible by 2^(levels - 1), the coarsest level at least 8 x 8");
    if (max_points < 1 || max_points > EDS_CT_MAX_POINTS || max_tries < 1 || max_tries > 4096)
        return fail(EDS_ERR_INVALID, "max_points is 1 .. 65536, max_tries 1 .. 4096");
    eds_ct* h = new eds_ct;
    if (int rc = h->own.open(device)) { delete h; return rc; }
    h->max_points = max_points; h->max_tries = max_tries;
    edsct::make_shape(h->geo, H, W, levels);
    h->prm = edsct::params_default();
    h->ph.exposure_ref = h->ph.exposure_new = 1.0f; h->ph.ref_a = h->ph.ref_b = 0.0;
    h->max_blocks = (int)blocks(H * W);
    const size_t tot = (size_t)h->geo.total, px0 = (size_t)H * W, mp = (size_t)max_points;
    const bool ok = h->own.alloc({{(void**)&h->d_geo, sizeof(Geo)},
                                  {(void**)&h->ref_px, tot * sizeof(Px)},
                                  {(void**)&h->new_px, tot * sizeof(Px)},
                                  {(void**)&h->idA, tot * sizeof(float)},
                                  {(void**)&h->wsA, tot * sizeof(float)},
                                  {(void**)&h->idB, tot * sizeof(float)},
                                  {(void**)&h->wsB, tot * sizeof(float)},
                                  {(void**)&h->pc, tot * sizeof(Pc)},
                                  {(void**)&h->d_pc_n, 8 * sizeof(int32_t)},
                                  {(void**)&h->block_cnt, (size_t)h->max_blocks * sizeof(int32_t)},
                                  {(void**)&h->first, px0 * sizeof(int32_t)},
                                  {(void**)&h->last, px0 * sizeof(int32_t)},
                                  {(void**)&h->pix, mp * sizeof(int32_t)},
                                  {(void**)&h->dropped, sizeof(int32_t)},
                                  {(void**)&h->in_img, px0 * sizeof(float)},
                                  {(void**)&h->in_cp, mp * 3 * sizeof(float)},
                                  {(void**)&h->in_hdif, mp * sizeof(float)},
                                  {(void**)&h->wgt, mp * sizeof(float)},
                                  {(void**)&h->d_out, (size_t)max_tries * sizeof(TrackOut)},
                                  {(void**)&h->d_T, (size_t)max_tries * 12 * sizeof(double)},
                                  {(void**)&h->d_aff, (size_t)max_tries * 2 * sizeof(double)},
                                  {(void**)&h->d_min_res, 5 * sizeof(double)},
                                  {(void**)&h->d_calc, 78 * sizeof(double)},
                                  {(void**)&h->d_rows, px0 * sizeof(Term)}});
    if (!ok || hipMemsetAsync(h->d_pc_n, 0, 8 * sizeof(int32_t), h->own.st) != hipSuccess || hipStreamSynchronize(h->own.st) != hipSuccess) {
        (void)hipGetLastError();
        eds_ct_destroy(h);
        return fail(EDS_ERR_HIP, "eds_ct_create: the device refused a stream or an allocation");
    }
    *ct = h;
    return EDS_OK;
}

void eds_ct_destroy(eds_ct* h) {
    if (!h) return;
    h->own.close();
    delete h;
}

int eds_ct_set_params(eds_ct* h, const eds_ct_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null parameters");
    Params s;
    std::memcpy(&s, p, sizeof(s));
    if (!edsct::params_valid(s)) return fail(EDS_ERR_INVALID, "parameters: every float finite; huber_th and coarse_cutoff_th > 0");
    h->prm = s;
    return EDS_OK;
}

int eds_ct_get_params(const eds_ct* h, eds_ct_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(p, &h->prm, sizeof(*p));
    return EDS_OK;
}

int eds_ct_set_calib(eds_ct* h, float fx, float fy, float cx, float cy) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (!edscapi::check_calib(fx, fy, cx, cy)) return fail(EDS_ERR_INVALID, "calibration: fx, fy, cx, cy finite, fx and fy > 0");
    Geo g = h->geo;
    edsct::make_k(g, fx, fy, cx, cy);
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_geo, &g, sizeof(g), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->geo = g;
    h->calib_set = true;
    return EDS_OK;
}

int eds_ct_get_k(const eds_ct* h, int lvl, float* K) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (!K) return fail(EDS_ERR_INVALID, "null output");
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_ct: no calibration set");
    const Level& L = h->geo.l[lvl];
    K[0] = L.fx; K[1] = L.fy; K[2] = L.cx; K[3] = L.cy;
    return EDS_OK;
}

int eds_ct_set_ref(eds_ct* h, const float* image, int64_t row_stride, int on_device, float exposure, double aff_a, double aff_b, int n,
                   const float* center_projected, const float* hdif, int32_t* pc_n_out, int32_t* dropped_out) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_ct: no calibration set");
    if (n < 0 || n > h->max_points) return fail(EDS_ERR_INVALID, std::to_string(n) + " contributions, the handle holds 0 .. " + std::to_string(h->max_points));
    if (n > 0 && (!center_projected || !hdif)) return fail(EDS_ERR_INVALID, "center_projected and hdif are required");
    if (!std::isfinite(exposure) || !std::isfinite(aff_a) || !std::isfinite(aff_b)) return fail(EDS_ERR_INVALID, "exposure and the affine pair must be finite");
    if (int rc = edscapi::check_images(h->own.dev, h->geo.H, h->geo.W, 1, image, &row_stride, nullptr, on_device, "image")) return rc;
    h->ref_set = false;
    if (int rc = load_frame(h, h->ref_px, image, row_stride, on_device)) return rc;
    const Geo& g = h->geo;
    const size_t px0 = (size_t)g.W * g.H;
    EDS_HIP_TRY(hipMemsetAsync(h->idA, 0, px0 * sizeof(float), h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->wsA, 0, px0 * sizeof(float), h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->first, 0x7f, px0 * sizeof(int32_t), h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->last, 0xff, px0 * sizeof(int32_t), h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->dropped, 0, sizeof(int32_t), h->own.st));
    if (n > 0) {
        EDS_HIP_TRY(hipMemcpyAsync(h->in_cp, center_projected, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->in_hdif, hdif, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        for (int pass = 0; pass < 2; ++pass)
            hipLaunchKernelGGL(k_ct_splat, dim3(blocks(n)), dim3(TB), 0, h->own.st, pass, n, h->in_cp, h->in_hdif, g.W, g.H, h->pix, h->wgt, h->first,
                               h->last, h->dropped, h->idA, h->wsA);
    }
    for (int l = 1; l < g.levels; ++l)
        hipLaunchKernelGGL(k_ct_levels, dim3(blocks(g.l[l].w * g.l[l].h)), dim3(TB), 0, h->own.st, h->idA, h->wsA, h->d_geo, l);
    for (int l = 0; l < g.levels; ++l) {
        const unsigned nb = blocks(g.l[l].w * g.l[l].h);
        hipLaunchKernelGGL(k_ct_dilate, dim3(nb), dim3(TB), 0, h->own.st, h->idA, h->wsA, h->idB, h->wsB, h->ref_px, h->d_geo, l, h->block_cnt);
        hipLaunchKernelGGL(k_ct_select, dim3(nb), dim3(TB), 0, h->own.st, h->idB, h->ref_px, h->pc, h->d_pc_n, h->block_cnt, h->d_geo, l);
    }
    EDS_HIP_TRY(hipGetLastError());
    int32_t back[6] = {0, 0, 0, 0, 0, 0};
    EDS_HIP_TRY(hipMemcpyAsync(back, h->d_pc_n, 5 * sizeof(int32_t), hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(back + 5, h->dropped, sizeof(int32_t), hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    for (int l = 0; l < edsct::MAX_LEVELS; ++l) h->pc_n[l] = l < g.levels ? back[l] : 0;
    if (pc_n_out) for (int l = 0; l < g.levels; ++l) pc_n_out[l] = back[l];
    if (dropped_out) *dropped_out = back[5];
    h->ph.exposure_ref = exposure; h->ph.ref_a = aff_a; h->ph.ref_b = aff_b;
    h->ref_set = true;
    return EDS_OK;
}

int eds_ct_set_new(eds_ct* h, const float* image, int64_t row_stride, int on_device, float exposure) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (!std::isfinite(exposure)) return fail(EDS_ERR_INVALID, "exposure must be finite");
    if (int rc = edscapi::check_images(h->own.dev, h->geo.H, h->geo.W, 1, image, &row_stride, nullptr, on_device, "image")) return rc;
    h->new_set = false;
    if (int rc = load_frame(h, h->new_px, image, row_stride, on_device)) return rc;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->ph.exposure_new = exposure;
    h->new_set = true;
    return EDS_OK;
}

int eds_ct_track(eds_ct* h, int count, const double* T_init, const double* aff_init, int coarsest_lvl, const double* min_res_for_abort,
                 eds_ct_result* results) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (count < 1 || count > h->max_tries) return fail(EDS_ERR_INVALID, std::to_string(count) + " tries, the handle holds 1 .. " + std::to_string(h->max_tries));
    if (!T_init || !aff_init || !min_res_for_abort || !results) return fail(EDS_ERR_INVALID, "T_init, aff_init, min_res_for_abort and results are required");
    if (int rc = check_level(h, coarsest_lvl)) return rc;
    if (!all_finite_d(T_init, 12 * count) || !all_finite_d(aff_init, 2 * count)) return fail(EDS_ERR_INVALID, "T_init or aff_init is not finite");
    if (int rc = check_ready(h)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_T, T_init, (size_t)count * 12 * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_aff, aff_init, (size_t)count * 2 * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_min_res, min_res_for_abort, 5 * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->d_out, 0, (size_t)count * sizeof(TrackOut), h->own.st));
    hipLaunchKernelGGL(k_ct_track, dim3((unsigned)count), dim3(edsct::LANES), 0, h->own.st, h->d_geo, h->prm, h->ph, h->new_px, h->pc, h->d_pc_n, h->d_T,
                       h->d_aff, coarsest_lvl, h->d_min_res, h->d_out);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<TrackOut> back((size_t)count);
    EDS_HIP_TRY(hipMemcpyAsync(back.data(), h->d_out, back.size() * sizeof(TrackOut), hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    std::memcpy(results, back.data(), back.size() * sizeof(TrackOut));
    return EDS_OK;
}

int eds_ct_calc_res(eds_ct* h, int lvl, const double* T, const double* aff, float cutoff, double* rs_out, double* H_out, double* b_out,
                    eds_ct_row* rows_out) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (!T || !aff) return fail(EDS_ERR_INVALID, "T and aff are required");
    if (!all_finite_d(T, 12) || !all_finite_d(aff, 2) || !std::isfinite(cutoff)) return fail(EDS_ERR_INVALID, "T, aff or the cutoff is not finite");
    if (int rc = check_ready(h)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_T, T, 12 * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_aff, aff, 2 * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    hipLaunchKernelGGL(k_ct_calc, dim3(1), dim3(edsct::LANES), 0, h->own.st, h->d_geo, h->prm, h->ph, h->new_px, h->pc, h->d_pc_n, lvl, h->d_T, h->d_aff,
                       cutoff, h->d_calc);
    const int n = h->pc_n[lvl];
    if (rows_out && n > 0)
        hipLaunchKernelGGL(k_ct_rows, dim3(blocks(n)), dim3(TB), 0, h->own.st, h->d_geo, h->prm, h->ph, h->new_px, h->pc, h->d_pc_n, lvl, h->d_T,
                           h->d_aff, cutoff, h->d_rows);
    EDS_HIP_TRY(hipGetLastError());
    double back[78];
    std::vector<Term> rows(rows_out ? (size_t)n : 0);
    EDS_HIP_TRY(hipMemcpyAsync(back, h->d_calc, sizeof(back), hipMemcpyDeviceToHost, h->own.st));
    if (!rows.empty()) EDS_HIP_TRY(hipMemcpyAsync(rows.data(), h->d_rows, rows.size() * sizeof(Term), hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    if (rs_out) std::memcpy(rs_out, back, 6 * sizeof(double));
    if (H_out) std::memcpy(H_out, back + 6, 64 * sizeof(double));
    if (b_out) std::memcpy(b_out, back + 70, 8 * sizeof(double));
    if (!rows.empty()) std::memcpy(rows_out, rows.data(), rows.size() * sizeof(Term));
    return EDS_OK;
}

int eds_ct_get_level(eds_ct* h, int which, int lvl, float* out, int32_t* n_out) {
    if (int rc = edscapi::check_handle(h, "eds_ct")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (which < EDS_CT_REF_IMAGE || which > EDS_CT_PC) return fail(EDS_ERR_INVALID, "which is EDS_CT_REF_IMAGE .. EDS_CT_PC");
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (which == EDS_CT_NEW_IMAGE ? !h->new_set : !h->ref_set) return fail(EDS_ERR_STATE, "eds_ct: that frame was never set");
    const Level& L = h->geo.l[lvl];
    const size_t px = (size_t)L.w * L.h;
    if (which == EDS_CT_REF_IMAGE || which == EDS_CT_NEW_IMAGE) {
        std::vector<Px> p(px);
        if (int rc = edscapi::read_back(h->own, p.data(), (which == EDS_CT_REF_IMAGE ? h->ref_px : h->new_px) + L.off, px * sizeof(Px))) return rc;
        for (size_t i = 0; i < px; ++i) { out[3 * i] = p[i].c; out[3 * i + 1] = p[i].dx; out[3 * i + 2] = p[i].dy; }
        if (n_out) *n_out = (int32_t)px;
    } else if (which == EDS_CT_IDEPTH || which == EDS_CT_WEIGHT_SUMS) {
        std::vector<float> p(px);
        if (int rc = edscapi::read_back(h->own, p.data(), (which == EDS_CT_IDEPTH ? h->idB : h->wsB) + L.off, px * sizeof(float))) return rc;
        std::memcpy(out, p.data(), px * sizeof(float));
        if (n_out) *n_out = (int32_t)px;
    } else {
        const size_t n = (size_t)h->pc_n[lvl];
        std::vector<Pc> p(n);
        if (int rc = edscapi::read_back(h->own, p.data(), h->pc + L.off, n * sizeof(Pc))) return rc;
        if (n) std::memcpy(out, p.data(), n * sizeof(Pc));
        if (n_out) *n_out = (int32_t)n;
    }
    return EDS_OK;
}

}  // extern "C"
