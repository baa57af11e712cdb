// include/eds_hip_winedit.h: the window's tables edited on the device.  The rules are eds_winedit.hpp, shared with the host; this file
// holds the kernels and the C entry points.  Everything of one call runs in the window's stream, in order.
//
// One edit is: the keep flags of the residuals (and of the points), an exclusive prefix sum of each — k_wed_tile_sums adds the flags
// of every tile of 1 024 rows, k_wed_tile_offsets (one workgroup) turns the sums into offsets, k_wed_number numbers the rows of a tile
// and scatters new -> old —, then the gathers: k_wed_words moves every narrow column a word a lane, k_wed_wide moves J and ef_J in
// 16-byte pieces, 19 consecutive lanes a row, so that a wavefront stores 64 consecutive pieces.  The flags and the two totals come back
// to the host for its copies of the tables; no row does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_device.h"
#include "../../include/eds_hip_winedit.h"
#include "../../include/eds_hip_activate.h"
#include "eds_capi_internal.hpp"
#include "eds_immature_internal.hpp"
#include "eds_window_internal.hpp"
#include "eds_winedit.hpp"
#include "eds_winflag.hpp"

using edscapi::blocks;
using edscapi::fail;
using edswed::Cols;
using edswed::SCAN_ITEMS;
using edswed::SCAN_TB;
using edswed::SCAN_TILE;

static_assert(edswed::WIDE_WORDS == edswin::J_WORDS && edswed::MAX_FRAMES == edswin::MAX_FRAMES && edswed::ST_IN == edswin::ST_IN, "eds_window.hpp's constants");
static_assert(edswed::FATE_ACTIVATED == edsact::ACTIVATED && edswed::ST_IN == edsact::ST_IN && edswed::ST_OUTLIER == edswin::ST_OUTLIER, "eds_activate.hpp's constants");
static_assert(sizeof(edswin::Point) % 4 == 0 && sizeof(edswin::PointOut) % 4 == 0, "the rows move by 32-bit words");

namespace {

constexpr int TB = 256;
constexpr int MAX_N = edswed::MAX_N, MARG_IN = MAX_N * (MAX_N + 1) + 16, MARG_WORDS = 2 * MARG_IN;   // HM, bM, prior, delta_prior; then HM', bM'

__global__ void __launch_bounds__(TB) k_wed_keep_residuals(int m, const int32_t* __restrict__ select, const int32_t* __restrict__ state,
                                                           int32_t* __restrict__ keep) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m) keep[r] = edswed::keep_residual(select, state, r);
}
__global__ void __launch_bounds__(TB) k_wed_keep_points(int n, const int32_t* __restrict__ flag, int32_t* __restrict__ keep) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n) keep[p] = edswed::keep_point(flag, p);
}
__global__ void __launch_bounds__(TB) k_wed_keep_residuals_of(int m, const int32_t* __restrict__ keep_p, const int32_t* __restrict__ res_point,
                                                              int32_t* __restrict__ keep) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m) keep[r] = edswed::keep_residual_of(keep_p, res_point, r);
}

// the inclusive sum over the workgroup's SCAN_TB values, every lane its own
__device__ inline int block_inclusive(int v, int32_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 1; s < SCAN_TB; s <<= 1) {
        const int add = t >= s ? sh[t - s] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int out = sh[t];
    __syncthreads();
    return out;
}

__global__ void __launch_bounds__(SCAN_TB) k_wed_tile_sums(const int32_t* __restrict__ keep, int n, int32_t* __restrict__ tile) {
    __shared__ int32_t sh[SCAN_TB];
    const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    int v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) if (base + k < n) v += keep[base + k] != 0;
    const int incl = block_inclusive(v, sh);
    if (threadIdx.x == SCAN_TB - 1) tile[blockIdx.x] = incl;
}

// one workgroup: tile[b] becomes the kept rows before tile b, *total all of them
__global__ void __launch_bounds__(SCAN_TB) k_wed_tile_offsets(int32_t* tile, int tiles, int32_t* total) {
    __shared__ int32_t sh[SCAN_TB];
    __shared__ int32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < tiles; base += SCAN_TB) {
        const int i = base + (int)threadIdx.x;
        const int v = i < tiles ? tile[i] : 0;
        const int incl = block_inclusive(v, sh);
        const int c = carry;
        __syncthreads();
        if (i < tiles) tile[i] = c + incl - v;
        if (threadIdx.x == SCAN_TB - 1) carry = c + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// excl[i] for every row of the tile, excl[n] by the lane that holds row n - 1, map[new] = old for the kept rows
__global__ void __launch_bounds__(SCAN_TB) k_wed_number(const int32_t* __restrict__ keep, int n, const int32_t* __restrict__ tile, int32_t* __restrict__ excl,
                                                        int32_t* __restrict__ map) {
    __shared__ int32_t sh[SCAN_TB];
    const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    int k4[SCAN_ITEMS], v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { k4[k] = base + k < n ? keep[base + k] != 0 : 0; v += k4[k]; }
    int run = tile[blockIdx.x] + block_inclusive(v, sh) - v;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const int i = base + k;
        if (i >= n) break;
        excl[i] = run;
        if (k4[k]) map[run] = i;                                // run < the kept rows <= n: inside map
        run += k4[k];
        if (i == n - 1) excl[n] = run;
    }
}

__global__ void __launch_bounds__(TB) k_wed_words(Cols t, const int32_t* __restrict__ map, int64_t words) {
    const int64_t g = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (g < words) edswed::move_word(t, map, g);
}
__global__ void __launch_bounds__(TB) k_wed_wide(const char* __restrict__ src, char* __restrict__ dst, const int32_t* __restrict__ map, int64_t pieces) {
    const int64_t g = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (g < pieces) edswed::move_wide(src, dst, map, g);
}
__global__ void __launch_bounds__(TB) k_wed_res_point(int m_new, const int32_t* __restrict__ res_point, const int32_t* __restrict__ map_r,
                                                      const int32_t* __restrict__ new_point, int32_t* __restrict__ out) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < m_new) out[i] = edswed::moved_res_point(res_point, map_r, new_point, i);
}
__global__ void __launch_bounds__(TB) k_wed_res_first(int n_new, int m_new, const int32_t* __restrict__ res_first, const int32_t* __restrict__ map_p,
                                                      const int32_t* __restrict__ excl_r, int32_t* __restrict__ out) {
    const int q = blockIdx.x * TB + threadIdx.x;
    if (q <= n_new) out[q] = edswed::moved_res_first(res_first, map_p, excl_r, q, n_new, m_new);
}

__global__ void __launch_bounds__(TB) k_wed_keep_not_towards(int m, const int32_t* __restrict__ res_target, int frame, int32_t* __restrict__ keep) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m) keep[r] = edswed::keep_residual_not_towards(res_target, frame, r);
}
// hosts and targets above the frame that left go down by one, each entry by its own lane
// ... and, where the history columns exist, the targets lastResiduals names (last_target NULL: they do not)
__global__ void __launch_bounds__(TB) k_wed_frames_down(int n, int m, int frame, edswin::Point* __restrict__ pts, int32_t* __restrict__ res_target,
                                                        int32_t* __restrict__ last_target) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < n) pts[i].host = edswed::frame_after(pts[i].host, frame);
    if (i < m) res_target[i] = edswed::frame_after(res_target[i], frame);
    if (last_target && i < n) {
        last_target[2 * i] = edswfl::target_after(last_target[2 * i], frame);
        last_target[2 * i + 1] = edswfl::target_after(last_target[2 * i + 1], frame);
    }
}
// The history columns of include/eds_hip_winflag.h (only launched once they exist).  A residual that leaves while its point stays:
// lastResiduals of the point no longer names it.  A point's residuals have distinct targets, so no two lanes store to one word.
__global__ void __launch_bounds__(TB) k_wed_forget(int m, const int32_t* __restrict__ keep, const int32_t* __restrict__ res_point,
                                                   const int32_t* __restrict__ res_target, int32_t* __restrict__ last_target) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m && !keep[r]) edswfl::forget_residual(last_target, res_point[r], res_target[r]);
}

struct DevSync { __device__ void operator()() const { __syncthreads(); } };
// marginalizeFrame's arithmetic: one workgroup, the matrix in LDS (edswed::marg_frame_body states every step)
__global__ void __launch_bounds__(TB) k_wed_marg_frame(edswed::MargIo io) {
    __shared__ edswed::MargMem mem;
    edswed::marg_frame_body(io, mem, (int)threadIdx.x, TB, DevSync());
}

// ---- eds_wed_insert_activated ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) k_wed_ins_flags(edswed::ImmCounts nn, int F, int mp, int stride, const int32_t* __restrict__ fate,
                                                      const int32_t* __restrict__ res_state, int32_t* __restrict__ keep_c, int32_t* __restrict__ keep_g) {
    const int64_t g = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (g >= (int64_t)F * mp * F) return;
    keep_g[g] = edswed::ins_keep_cell(nn, fate, res_state, F, mp, stride, g);
    if (g % F == 0) keep_c[g / F] = edswed::ins_keep_candidate(nn, fate, mp, (int)(g / F));
}
// the window's own rows: where they go (map new -> old), their first residual and their point under the new numbering
__global__ void __launch_bounds__(TB) k_wed_ins_old(edswed::Ins s, int n, int m, const edswin::Point* __restrict__ pts, const int32_t* __restrict__ res_point,
                                                    int32_t* __restrict__ map_p, int32_t* __restrict__ map_r, int32_t* __restrict__ res_first_new,
                                                    int32_t* __restrict__ res_point_new) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < n) {
        const int host = pts[i].host, q = edswed::ins_old_point(s, i, host);
        map_p[q] = i;
        res_first_new[q] = edswed::ins_old_res(s, s.res_first[i], host);
    }
    if (i < m) {
        const int p = res_point[i], host = pts[p].host, r = edswed::ins_old_res(s, i, host);
        map_r[r] = i;
        res_point_new[r] = edswed::ins_old_point(s, p, host);
    }
}
// activated point k (candidate map_c[k]): its row as eds_act_get_activated returns it, zeros elsewhere (the gather wrote them)
__global__ void __launch_bounds__(TB) k_wed_ins_new_points(edswed::Ins s, int K, const int32_t* __restrict__ map_c, const edsimm::Point* __restrict__ imm,
                                                           const float* __restrict__ fit, float scale, edswin::Point* __restrict__ pts, float* __restrict__ ids,
                                                           float* __restrict__ idz, int32_t* __restrict__ res_first_new) {
    const int k = blockIdx.x * TB + threadIdx.x;
    if (k >= K) return;
    const int c = map_c[k], q = edswed::ins_new_point(s, c);
    const edsimm::Point& a = imm[c];
    edswin::Point o;
    o.host = c / s.mp; o.u = a.u; o.v = a.v;
#pragma unroll
    for (int j = 0; j < 8; ++j) { o.color[j] = a.color[j]; o.weights[j] = a.weights[j]; }
    pts[q] = o;
    const float d = fit[4 * (size_t)c] * scale;
    ids[q] = d; idz[q] = d;
    res_first_new[q] = edswed::ins_new_res(s, (int64_t)c * s.F);
}
// new residual j (grid cell map_g[j]): as eds_win_set_residuals leaves a residual with state IN and energy 0
__global__ void __launch_bounds__(TB) k_wed_ins_new_residuals(edswed::Ins s, int R, const int32_t* __restrict__ map_g, int32_t* __restrict__ res_point_new,
                                                              int32_t* __restrict__ res_target, int32_t* __restrict__ new_state) {
    const int j = blockIdx.x * TB + threadIdx.x;
    if (j >= R) return;
    const int64_t g = map_g[j];
    const int r = edswed::ins_new_res(s, g);
    res_point_new[r] = edswed::ins_new_point(s, (int)(g / s.F));
    res_target[r] = (int)(g % s.F);
    new_state[r] = edswed::ST_OUTLIER;
}
// ... and their history: lastResiduals from the cells towards the two latest frames, is_new on every new residual
__global__ void __launch_bounds__(TB) k_wed_ins_history(edswed::Ins s, int K, int R, const int32_t* __restrict__ map_c, const int32_t* __restrict__ map_g,
                                                        const int32_t* __restrict__ keep_g, edswfl::Hist hist) {
    const int k = blockIdx.x * TB + threadIdx.x;
    if (k < K) {
        const int c = map_c[k];
        edswfl::activated_point(hist, edswed::ins_new_point(s, c), s.F, keep_g[(int64_t)c * s.F + s.F - 1], keep_g[(int64_t)c * s.F + s.F - 2]);
    }
    if (k < R) hist.is_new[edswed::ins_new_res(s, map_g[k])] = 1;
}

int ensure_state(eds_win* h) {
    const size_t mp = (size_t)h->max_points, mr = (size_t)h->max_residuals, ms = mp > mr ? mp : mr, jw = edswin::J_WORDS;
    if (!h->wed) {
        eds_wed_state* s = new eds_wed_state;
        const bool ok = h->own.alloc({{(void**)&s->pts, mp * sizeof(edswin::Point)},
                                      {(void**)&s->ids, mp * sizeof(float)},
                                      {(void**)&s->idz, mp * sizeof(float)},
                                      {(void**)&s->prior, mp * sizeof(float)},
                                      {(void**)&s->delta, mp * sizeof(float)},
                                      {(void**)&s->lf, mp * 6 * sizeof(float)},
                                      {(void**)&s->pout, mp * sizeof(edswin::PointOut)},
                                      {(void**)&s->res_first, (mp + 1) * sizeof(int32_t)},
                                      {(void**)&s->res_point, mr * sizeof(int32_t)},
                                      {(void**)&s->res_target, mr * sizeof(int32_t)},
                                      {(void**)&s->state, mr * sizeof(int32_t)},
                                      {(void**)&s->new_state, mr * sizeof(int32_t)},
                                      {(void**)&s->active, mr * sizeof(int32_t)},
                                      {(void**)&s->energy, mr * sizeof(float)},
                                      {(void**)&s->new_energy, mr * sizeof(float)},
                                      {(void**)&s->new_energy_wo, mr * sizeof(float)},
                                      {(void**)&s->ret, mr * sizeof(float)},
                                      {(void**)&s->cp, mr * 3 * sizeof(float)},
                                      {(void**)&s->proj, mr * 16 * sizeof(float)},
                                      {(void**)&s->J, mr * jw * sizeof(float)},
                                      {(void**)&s->efJ, mr * jw * sizeof(float)},
                                      {(void**)&s->JpJdF, mr * 8 * sizeof(float)},
                                      {(void**)&s->flag, ms * sizeof(int32_t)},
                                      {(void**)&s->keep_r, mr * sizeof(int32_t)},
                                      {(void**)&s->excl_r, (mr + 1) * sizeof(int32_t)},
                                      {(void**)&s->map_r, mr * sizeof(int32_t)},
                                      {(void**)&s->keep_p, mp * sizeof(int32_t)},
                                      {(void**)&s->excl_p, (mp + 1) * sizeof(int32_t)},
                                      {(void**)&s->map_p, mp * sizeof(int32_t)},
                                      {(void**)&s->block, (ms / SCAN_TILE + 1) * sizeof(int32_t)},
                                      {(void**)&s->total, 4 * sizeof(int32_t)},
                                      {(void**)&s->marg, (size_t)MARG_WORDS * sizeof(double)}});
        if (!ok) {                                              // nothing half-allocated stays behind: the next call allocates again
            delete s;
            return fail(EDS_ERR_HIP, "eds_wed: the device refused an allocation for the second set of tables");
        }
        h->wed = s;
    }
    eds_wed_state* s = h->wed;
    if (h->wsv && !s->have_wsv) {
        const bool ok = h->own.alloc({{(void**)&s->lin, mr * sizeof(int32_t)},
                                      {(void**)&s->rtz, mr * 8 * sizeof(float)},
                                      {(void**)&s->res_approx, mr * 8 * sizeof(float)},
                                      {(void**)&s->step, mp * sizeof(float)},
                                      {(void**)&s->backup, mp * sizeof(float)}});
        if (!ok) return fail(EDS_ERR_HIP, "eds_wed: the device refused an allocation for the second set of the solver's rows");
        s->have_wsv = true;
    }
    return EDS_OK;
}

// the caller's flags into the scratch array (host memory, or device memory that eds_dev_check_range has passed)
int stage_flags(eds_win* h, const int32_t* flags, int on_device, size_t count) {
    if (!count) return EDS_OK;
    EDS_HIP_TRY(hipMemcpyAsync(h->wed->flag, flags, count * sizeof(int32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->own.st));
    return EDS_OK;
}

// the exclusive sums of keep[0 .. n): excl (n + 1 entries), map, total
int queue_scan(eds_win* h, const int32_t* keep, int n, int32_t* excl, int32_t* map, int32_t* total, int32_t* tile = nullptr) {
    if (!tile) tile = h->wed->block;
    if (!n) {
        EDS_HIP_TRY(hipMemsetAsync(excl, 0, sizeof(int32_t), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(total, 0, sizeof(int32_t), h->own.st));
        return EDS_OK;
    }
    const int tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(k_wed_tile_sums, dim3((unsigned)tiles), dim3(SCAN_TB), 0, h->own.st, keep, n, tile);
    hipLaunchKernelGGL(k_wed_tile_offsets, dim3(1), dim3(SCAN_TB), 0, h->own.st, tile, tiles, total);
    hipLaunchKernelGGL(k_wed_number, dim3((unsigned)tiles), dim3(SCAN_TB), 0, h->own.st, keep, n, tile, excl, map);
    EDS_HIP_TRY(hipGetLastError());
    return EDS_OK;
}

template <class T> void swap_ptr(T*& a, T*& b) { T* t = a; a = b; b = t; }

// every per-residual column but the point (and every per-point column but the first residual) of the new rows 0 .. rows - 1 into the
// second set: row i is row map[i] of the first set, or zeros where map[i] < 0
void queue_residual_rows(eds_win* h, const int32_t* map, int rows) {
    eds_wed_state* s = h->wed;
    eds_wsv_state* v = h->wsv;
    Cols t;
    edswed::cols_clear(t);
    edswed::cols_add(t, h->res_target, s->res_target, 1); edswed::cols_add(t, h->state, s->state, 1);
    edswed::cols_add(t, h->new_state, s->new_state, 1); edswed::cols_add(t, h->active, s->active, 1);
    edswed::cols_add(t, h->energy, s->energy, 1); edswed::cols_add(t, h->new_energy, s->new_energy, 1);
    edswed::cols_add(t, h->new_energy_wo, s->new_energy_wo, 1); edswed::cols_add(t, h->ret, s->ret, 1);
    edswed::cols_add(t, h->cp, s->cp, 3); edswed::cols_add(t, h->proj, s->proj, 16); edswed::cols_add(t, h->JpJdF, s->JpJdF, 8);
    if (v) { edswed::cols_add(t, v->lin, s->lin, 1); edswed::cols_add(t, v->rtz, s->rtz, 8); edswed::cols_add(t, v->res_approx, s->res_approx, 8); }
    if (const eds_wfl_state* f = h->wfl) edswed::cols_add(t, f->is_new, f->is_new2, 1);
    const int64_t words = (int64_t)rows * t.words, pieces = (int64_t)rows * edswed::WIDE_PIECES;
    hipLaunchKernelGGL(k_wed_words, dim3(blocks(words)), dim3(TB), 0, h->own.st, t, map, words);
    hipLaunchKernelGGL(k_wed_wide, dim3(blocks(pieces)), dim3(TB), 0, h->own.st, (const char*)h->J, (char*)s->J, map, pieces);
    hipLaunchKernelGGL(k_wed_wide, dim3(blocks(pieces)), dim3(TB), 0, h->own.st, (const char*)h->efJ, (char*)s->efJ, map, pieces);
}
void queue_point_rows(eds_win* h, const int32_t* map, int rows) {
    eds_wed_state* s = h->wed;
    eds_wsv_state* v = h->wsv;
    Cols t;
    edswed::cols_clear(t);
    edswed::cols_add(t, h->pts, s->pts, (int)(sizeof(edswin::Point) / 4)); edswed::cols_add(t, h->ids, s->ids, 1); edswed::cols_add(t, h->idz, s->idz, 1);
    edswed::cols_add(t, h->prior, s->prior, 1); edswed::cols_add(t, h->delta, s->delta, 1); edswed::cols_add(t, h->lf, s->lf, 6);
    edswed::cols_add(t, h->pout, s->pout, (int)(sizeof(edswin::PointOut) / 4));
    if (v) { edswed::cols_add(t, v->step, s->step, 1); edswed::cols_add(t, v->backup, s->backup, 1); }
    if (const eds_wfl_state* f = h->wfl) {
        edswed::cols_add(t, f->num_good, f->num_good2, 1); edswed::cols_add(t, f->max_rel_baseline, f->max_rel_baseline2, 1);
        edswed::cols_add(t, f->last_target, f->last_target2, 2); edswed::cols_add(t, f->last_state, f->last_state2, 2);
    }
    const int64_t words = (int64_t)rows * t.words;
    hipLaunchKernelGGL(k_wed_words, dim3(blocks(words)), dim3(TB), 0, h->own.st, t, map, words);
}
// the second set becomes the window's
void exchange_sets(eds_win* h, bool points_too) {
    eds_wed_state* s = h->wed;
    eds_wsv_state* v = h->wsv;
    eds_wfl_state* f = h->wfl;
    if (f) swap_ptr(f->is_new, f->is_new2);
    if (f && points_too) {
        swap_ptr(f->num_good, f->num_good2); swap_ptr(f->max_rel_baseline, f->max_rel_baseline2);
        swap_ptr(f->last_target, f->last_target2); swap_ptr(f->last_state, f->last_state2);
    }
    swap_ptr(h->res_target, s->res_target); swap_ptr(h->state, s->state); swap_ptr(h->new_state, s->new_state); swap_ptr(h->active, s->active);
    swap_ptr(h->energy, s->energy); swap_ptr(h->new_energy, s->new_energy); swap_ptr(h->new_energy_wo, s->new_energy_wo); swap_ptr(h->ret, s->ret);
    swap_ptr(h->cp, s->cp); swap_ptr(h->proj, s->proj); swap_ptr(h->JpJdF, s->JpJdF); swap_ptr(h->J, s->J); swap_ptr(h->efJ, s->efJ);
    swap_ptr(h->res_point, s->res_point); swap_ptr(h->res_first, s->res_first);
    if (v) { swap_ptr(v->lin, s->lin); swap_ptr(v->rtz, s->rtz); swap_ptr(v->res_approx, s->res_approx); }
    if (points_too) {
        swap_ptr(h->pts, s->pts); swap_ptr(h->ids, s->ids); swap_ptr(h->idz, s->idz); swap_ptr(h->prior, s->prior); swap_ptr(h->delta, s->delta);
        swap_ptr(h->lf, s->lf); swap_ptr(h->pout, s->pout);
        if (v) { swap_ptr(v->step, s->step); swap_ptr(v->backup, s->backup); }
    }
}

// keep_r (and keep_p when the points change) are on the device.  Numbers the rows, reads the flags and the totals back, moves every
// row into the second set, exchanges the sets and brings the host copies up to date.
int compact(eds_win* h, bool points_change, int32_t* removed_points, int32_t* removed_residuals) {
    eds_wed_state* s = h->wed;
    hipStream_t st = h->own.st;
    const int n = h->n, m = h->m;
    if (int rc = queue_scan(h, s->keep_r, m, s->excl_r, s->map_r, s->total)) return rc;
    if (points_change)
        if (int rc = queue_scan(h, s->keep_p, n, s->excl_p, s->map_p, s->total + 1)) return rc;
    std::vector<int32_t> keep_r((size_t)m), keep_p(points_change ? (size_t)n : 0);
    int32_t total[2] = {0, n};
    if (m) EDS_HIP_TRY(hipMemcpyAsync(keep_r.data(), s->keep_r, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (points_change && n) EDS_HIP_TRY(hipMemcpyAsync(keep_p.data(), s->keep_p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipMemcpyAsync(total, s->total, (points_change ? 2 : 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    if (!points_change) total[1] = n;
    edswed::Mirrors w;                                          // a copy: the window's own change once the rows have moved
    w.host_of = h->host_of; w.point = h->h_point; w.target = h->h_target;
    w.n = n; w.m = m;
    edswed::edit_mirrors(w, points_change ? keep_p.data() : nullptr, keep_r.data());
    const int m2 = w.m, n2 = w.n;
    if (total[0] != m2 || total[1] != n2)                       // the device's prefix sums and the host's count of the same flags
        return fail(EDS_ERR_HIP, "eds_wed: the device numbered " + std::to_string(total[0]) + " residuals and " + std::to_string(total[1]) + " points, the flags hold " +
                                     std::to_string(m2) + " and " + std::to_string(n2));
    // per residual
    if (h->wfl && !points_change && m)                          // a point that stays forgets the residuals that leave (one that leaves takes its history along)
        hipLaunchKernelGGL(k_wed_forget, dim3(blocks(m)), dim3(TB), 0, st, m, s->keep_r, h->res_point, h->res_target, h->wfl->last_target);
    if (m2) {
        queue_residual_rows(h, s->map_r, m2);
        hipLaunchKernelGGL(k_wed_res_point, dim3(blocks(m2)), dim3(TB), 0, st, m2, h->res_point, s->map_r, points_change ? s->excl_p : (const int32_t*)nullptr,
                           s->res_point);
    }
    hipLaunchKernelGGL(k_wed_res_first, dim3(blocks((int64_t)n2 + 1)), dim3(TB), 0, st, n2, m2, h->res_first, points_change ? s->map_p : (const int32_t*)nullptr,
                       s->excl_r, s->res_first);
    // per point
    if (points_change && n2) queue_point_rows(h, s->map_p, n2);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(st));
    exchange_sets(h, points_change);
    h->host_of.swap(w.host_of); h->h_point.swap(w.point); h->h_target.swap(w.target);
    h->n = n2; h->m = m2; h->max_host = w.max_host; h->max_target = w.max_target;
    if (h->wfl) h->wfl->fates_current = false;                  // the fates of include/eds_hip_winflag.h were decided for other tables
    if (removed_points) *removed_points = n - n2;
    if (removed_residuals) *removed_residuals = m - m2;
    return EDS_OK;
}

// what every edit checks before anything is queued
int check_flags(const eds_win* h, const int32_t* flags, int on_device, size_t count, bool required) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    if (!flags) return required && count ? fail(EDS_ERR_INVALID, "the flags are required") : (int)EDS_OK;
    if (on_device && count)
        if (int rc = eds_dev_check_range(h->own.dev, flags, count * sizeof(int32_t))) return rc;
    return EDS_OK;
}

}  // namespace

namespace edswin_internal {

void wed_release(eds_win* h) {
    delete h->wed;
    h->wed = nullptr;
}
int wed_ensure_state(eds_win* h) { return ensure_state(h); }
int wed_queue_scan(eds_win* h, const int32_t* keep, int n, int32_t* excl, int32_t* map, int32_t* total) { return queue_scan(h, keep, n, excl, map, total); }
void wed_queue_residual_rows(eds_win* h, const int32_t* map, int rows) { queue_residual_rows(h, map, rows); }
void wed_exchange_residual_sets(eds_win* h) { exchange_sets(h, false); }

}  // namespace edswin_internal

extern "C" {

int eds_wed_abi_version(void) { return EDS_HIP_WINEDIT_ABI_VERSION; }

int eds_wed_remove_residuals(eds_win* h, const int32_t* select, int on_device, int32_t* removed_out) {
    if (int rc = check_flags(h, select, on_device, h ? (size_t)h->m : 0, false)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    if (select)
        if (int rc = stage_flags(h, select, on_device, (size_t)h->m)) return rc;
    if (h->m)
        hipLaunchKernelGGL(k_wed_keep_residuals, dim3(blocks(h->m)), dim3(TB), 0, h->own.st, h->m, select ? h->wed->flag : (const int32_t*)nullptr, h->state,
                           h->wed->keep_r);
    return compact(h, false, nullptr, removed_out);
}

int eds_wed_remove_points(eds_win* h, const int32_t* flag, int on_device, int32_t* removed_points_out, int32_t* removed_residuals_out) {
    if (int rc = check_flags(h, flag, on_device, h ? (size_t)h->n : 0, true)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    if (int rc = stage_flags(h, flag, on_device, (size_t)h->n)) return rc;
    if (h->n) hipLaunchKernelGGL(k_wed_keep_points, dim3(blocks(h->n)), dim3(TB), 0, h->own.st, h->n, h->wed->flag, h->wed->keep_p);
    if (h->m) hipLaunchKernelGGL(k_wed_keep_residuals_of, dim3(blocks(h->m)), dim3(TB), 0, h->own.st, h->m, h->wed->keep_p, h->res_point, h->wed->keep_r);
    return compact(h, true, removed_points_out, removed_residuals_out);
}

int eds_wed_marginalize_frame(eds_win* h, int frame, const double* prior, const double* delta_prior, const double* HM, const double* bM, double* HM_out,
                              double* bM_out) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!prior || !delta_prior || !HM || !bM || !HM_out || !bM_out) return fail(EDS_ERR_INVALID, "prior, delta_prior, HM, bM, HM_out and bM_out are required");
    if (!h->wsv || !h->wsv->valid)
        return fail(EDS_ERR_STATE, "eds_wed_marginalize_frame: no eds_wsv state set (the reference asserts EFDeltaValid and EFAdjointsValid); F is that state's");
    const int F = h->wsv->F, N = 4 + 8 * F, nd = N - 8;
    if (F < 3 || F > EDS_WIN_MAX_FRAMES) return fail(EDS_ERR_INVALID, "eds_wed_marginalize_frame: F is 3 .. 8");
    if (frame < 0 || frame >= F) return fail(EDS_ERR_INVALID, "frame " + std::to_string(frame) + " of " + std::to_string(F));
    const size_t NN = (size_t)N * N;
    for (size_t i = 0; i < NN; ++i) if (!std::isfinite(HM[i])) return fail(EDS_ERR_INVALID, "eds_wed_marginalize_frame: HM is not finite");
    for (int i = 0; i < N; ++i) if (!std::isfinite(bM[i])) return fail(EDS_ERR_INVALID, "eds_wed_marginalize_frame: bM is not finite");
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(prior[k]) || !std::isfinite(delta_prior[k])) return fail(EDS_ERR_INVALID, "eds_wed_marginalize_frame: a prior is not finite");
    for (int32_t host : h->host_of)
        if (host == frame) return fail(EDS_ERR_STATE, "eds_wed_marginalize_frame: a point is still hosted by frame " + std::to_string(frame) + " (the reference asserts)");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    eds_wed_state* s = h->wed;
    hipStream_t st = h->own.st;
    // the arithmetic first: when it refuses, nothing has changed
    std::vector<double> in((size_t)MARG_IN), out((size_t)nd * (nd + 1));
    std::memcpy(in.data(), HM, NN * sizeof(double));
    std::memcpy(in.data() + NN, bM, (size_t)N * sizeof(double));
    std::memcpy(in.data() + NN + N, prior, 8 * sizeof(double));
    std::memcpy(in.data() + NN + N + 8, delta_prior, 8 * sizeof(double));
    int32_t bad = 0;
    EDS_HIP_TRY(hipMemcpyAsync(s->marg, in.data(), (NN + N + 16) * sizeof(double), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipMemsetAsync(s->total + 2, 0, sizeof(int32_t), st));
    const edswed::MargIo io = {N, frame, s->marg, s->marg + NN, s->marg + NN + N, s->marg + NN + N + 8, s->marg + MARG_IN, s->marg + MARG_IN + (size_t)nd * nd,
                               s->total + 2};
    hipLaunchKernelGGL(k_wed_marg_frame, dim3(1), dim3(TB), 0, st, io);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipMemcpyAsync(out.data(), s->marg + MARG_IN, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipMemcpyAsync(&bad, s->total + 2, sizeof(bad), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(EDS_ERR_NOT_USABLE, "eds_wed_marginalize_frame: the frame's scaled 8 x 8 block has a zero pivot, or the result is not finite; nothing changed");
    // the tables: every residual towards the frame goes, the frames above it go down by one, their image planes one slot
    if (h->m) hipLaunchKernelGGL(k_wed_keep_not_towards, dim3(blocks(h->m)), dim3(TB), 0, st, h->m, h->res_target, frame, s->keep_r);
    if (int rc = compact(h, false, nullptr, nullptr)) return rc;
    const int most = h->n > h->m ? h->n : h->m;
    if (most) hipLaunchKernelGGL(k_wed_frames_down, dim3(blocks(most)), dim3(TB), 0, st, h->n, h->m, frame, h->pts, h->res_target,
                                 h->wfl ? h->wfl->last_target : (int32_t*)nullptr);
    EDS_HIP_TRY(hipGetLastError());
    const size_t px = (size_t)h->H * h->W;
    for (int f = frame + 1; f < F; ++f)
        EDS_HIP_TRY(hipMemcpyAsync(h->frames + (size_t)(f - 1) * px, h->frames + (size_t)f * px, px * sizeof(edswin::Px), hipMemcpyDeviceToDevice, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    uint32_t set = h->frames_set & ~((1u << F) - 1u);           // slots from F on are not the window's
    for (int f = 0; f < F; ++f)
        if (f != frame && (h->frames_set >> f & 1u)) set |= 1u << edswed::frame_after(f, frame);
    h->frames_set = set;
    h->max_host = h->max_target = -1;
    for (int32_t& host : h->host_of) { host = edswed::frame_after(host, frame); if (host > h->max_host) h->max_host = host; }
    for (int32_t& t : h->h_target) { t = edswed::frame_after(t, frame); if (t > h->max_target) h->max_target = t; }
    // F changed: the state is to be set again (eds_wed_set_state keeps priorF, isLinearized and res_toZeroF: rows_live stays)
    eds_wsv_state* v = h->wsv;
    v->valid = false; v->lf_on_device = false; v->have_backup = false; v->have_step = false; v->have_system = false;
    std::memcpy(HM_out, out.data(), (size_t)nd * nd * sizeof(double));
    std::memcpy(bM_out, out.data() + (size_t)nd * nd, (size_t)nd * sizeof(double));
    return EDS_OK;
}

int eds_wed_set_state(eds_win* h, int F, const double* adHost, const double* adTarget, const double* delta, const double* prior,
                      const double* delta_prior, const double* cPrior, const double* cDelta) {
    return edswin_internal::wsv_set_state(h, F, adHost, adTarget, delta, prior, delta_prior, cPrior, cDelta, nullptr, nullptr, true);
}

int eds_wed_insert_activated(eds_win* h, eds_imm* im, int32_t* inserted_points_out, int32_t* inserted_residuals_out) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!im) return fail(EDS_ERR_INVALID, "null eds_imm handle");
    if (im->own.dev != h->own.dev) return fail(EDS_ERR_INVALID, "eds_wed_insert_activated: the eds_imm lives on another device");
    if (im->H != h->H || im->W != h->W) return fail(EDS_ERR_INVALID, "eds_wed_insert_activated: the eds_imm's H x W is not the window's");
    if (!im->act || !im->act->fit_valid) return fail(EDS_ERR_STATE, "eds_wed_insert_activated: no fit (eds_act_optimize first)");
    const eds_act_state* a = im->act;
    int frames = 0;
    while (frames < h->max_frames && (h->frames_set >> frames & 1u)) ++frames;
    const int F = a->sel_hosts, mp = im->max_points;
    if (F != frames || F < 2 || F > EDS_WIN_MAX_FRAMES)
        return fail(EDS_ERR_INVALID, "eds_wed_insert_activated: the selection covers " + std::to_string(F) + " hosts, the window holds " + std::to_string(frames) + " frames");
    if (h->max_host >= F || h->max_target >= F) return fail(EDS_ERR_INVALID, "a point's host or a residual's target is not below F");
    const size_t C = (size_t)F * mp, G = C * F;
    if (G > ((size_t)1 << 30)) return fail(EDS_ERR_INVALID, "eds_wed_insert_activated: the eds_imm is too large");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    eds_wed_state* s = h->wed;
    hipStream_t st = h->own.st;
    if (s->ins_cap < C) {                                       // scratch for this eds_imm: C candidates, up to 8 C cells
        for (int32_t** p : {&s->ins_keep, &s->ins_excl_c, &s->ins_excl_g, &s->ins_map_c, &s->ins_map_g, &s->ins_tile, &s->ins_first}) h->own.release(*p);
        s->ins_cap = 0;
        const size_t C8 = (size_t)EDS_WIN_MAX_FRAMES * mp, G8 = C8 * EDS_WIN_MAX_FRAMES;
        if (!h->own.alloc({{(void**)&s->ins_keep, (C8 + G8) * sizeof(int32_t)}, {(void**)&s->ins_excl_c, (C8 + 1) * sizeof(int32_t)},
                           {(void**)&s->ins_excl_g, (G8 + 1) * sizeof(int32_t)}, {(void**)&s->ins_map_c, C8 * sizeof(int32_t)},
                           {(void**)&s->ins_map_g, G8 * sizeof(int32_t)}, {(void**)&s->ins_tile, (G8 / SCAN_TILE + 1) * sizeof(int32_t)},
                           {(void**)&s->ins_first, 9 * sizeof(int32_t)}}))
            return fail(EDS_ERR_HIP, "eds_wed_insert_activated: the device refused an allocation");
        s->ins_cap = C8;
    }
    int32_t *keep_c = s->ins_keep, *keep_g = s->ins_keep + C;
    edswed::ImmCounts nn;
    for (int f = 0; f < edswed::MAX_FRAMES; ++f) nn.n[f] = f < F ? im->n[f] : 0;
    // which candidates enter, which cells become residuals, and their ranks: nothing of the window is touched yet
    hipLaunchKernelGGL(k_wed_ins_flags, dim3(blocks((int64_t)G)), dim3(TB), 0, st, nn, F, mp, a->stride, a->fate, a->res_state, keep_c, keep_g);
    if (int rc = queue_scan(h, keep_c, (int)C, s->ins_excl_c, s->ins_map_c, s->total, s->ins_tile)) return rc;
    if (int rc = queue_scan(h, keep_g, (int)G, s->ins_excl_g, s->ins_map_g, s->total + 1, s->ins_tile)) return rc;
    std::vector<int32_t> flags(C + G);
    int32_t total[2] = {0, 0};
    EDS_HIP_TRY(hipMemcpyAsync(flags.data(), s->ins_keep, (C + G) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipMemcpyAsync(total, s->total, sizeof(total), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    const int n = h->n, m = h->m, K = total[0], R = total[1], n2 = n + K, m2 = m + R;
    if (n2 > h->max_points || m2 > h->max_residuals)
        return fail(EDS_ERR_STATE, "eds_wed_insert_activated: " + std::to_string(n2) + " points and " + std::to_string(m2) + " residuals do not fit the window's " +
                                       std::to_string(h->max_points) + " and " + std::to_string(h->max_residuals));
    // the host's copies by the same rules, from the flags
    std::vector<int32_t> excl_c(C + 1), excl_g(G + 1), map_c(C), map_g(G), first(9, n), res_first((size_t)n + 1, 0);
    if (edswed::scan_serial(flags.data(), (int)C, excl_c.data(), map_c.data()) != K || edswed::scan_serial(flags.data() + C, (int)G, excl_g.data(), map_g.data()) != R)
        return fail(EDS_ERR_HIP, "eds_wed_insert_activated: the device's prefix sums and the host's count of the same flags differ");
    for (int f = 0, p = 0; f < 9; ++f) { first[f] = p; while (p < n && h->host_of[p] == f) ++p; }
    for (int r = 0; r < m; ++r) ++res_first[h->h_point[r] + 1];
    for (int p = 0; p < n; ++p) res_first[p + 1] += res_first[p];
    const edswed::Ins hs = {F, mp, first.data(), res_first.data(), excl_c.data(), excl_g.data()};
    std::vector<int32_t> host_of((size_t)n2), h_point((size_t)m2), h_target((size_t)m2);
    for (int p = 0; p < n; ++p) host_of[edswed::ins_old_point(hs, p, h->host_of[p])] = h->host_of[p];
    for (int k = 0; k < K; ++k) host_of[edswed::ins_new_point(hs, map_c[k])] = map_c[k] / mp;
    for (int r = 0; r < m; ++r) {
        const int p = h->h_point[r], host = h->host_of[p], i = edswed::ins_old_res(hs, r, host);
        h_point[i] = edswed::ins_old_point(hs, p, host); h_target[i] = h->h_target[r];
    }
    for (int j = 0; j < R; ++j) {
        const int i = edswed::ins_new_res(hs, map_g[j]);
        h_point[i] = edswed::ins_new_point(hs, map_g[j] / F); h_target[i] = map_g[j] % F;
    }
    // the tables: old rows to their new places, new rows zero, then the new rows' own values
    const edswed::Ins ds = {F, mp, s->ins_first, h->res_first, s->ins_excl_c, s->ins_excl_g};
    EDS_HIP_TRY(hipMemcpyAsync(s->ins_first, first.data(), 9 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (n2) EDS_HIP_TRY(hipMemsetAsync(s->map_p, 0xff, (size_t)n2 * sizeof(int32_t), st));
    if (m2) EDS_HIP_TRY(hipMemsetAsync(s->map_r, 0xff, (size_t)m2 * sizeof(int32_t), st));
    const int most = n > m ? n : m;
    if (most) hipLaunchKernelGGL(k_wed_ins_old, dim3(blocks(most)), dim3(TB), 0, st, ds, n, m, h->pts, h->res_point, s->map_p, s->map_r, s->res_first, s->res_point);
    if (m2) queue_residual_rows(h, s->map_r, m2);
    if (n2) queue_point_rows(h, s->map_p, n2);
    if (K) hipLaunchKernelGGL(k_wed_ins_new_points, dim3(blocks(K)), dim3(TB), 0, st, ds, K, s->ins_map_c, im->points, a->fit, a->prm.scale_idepth, s->pts, s->ids, s->idz,
                              s->res_first);
    if (R) hipLaunchKernelGGL(k_wed_ins_new_residuals, dim3(blocks(R)), dim3(TB), 0, st, ds, R, s->ins_map_g, s->res_point, s->res_target, s->new_state);
    if (const eds_wfl_state* f = h->wfl) {                     // the second set's columns: exchange_sets makes them the window's
        const edswfl::Hist hist = {f->num_good2, f->max_rel_baseline2, f->last_target2, f->last_state2, f->is_new2};
        const int most_new = K > R ? K : R;
        if (most_new) hipLaunchKernelGGL(k_wed_ins_history, dim3(blocks(most_new)), dim3(TB), 0, st, ds, K, R, s->ins_map_c, s->ins_map_g, keep_g, hist);
    }
    EDS_HIP_TRY(hipGetLastError());
    const int32_t end = m2;
    EDS_HIP_TRY(hipMemcpyAsync(s->res_first + n2, &end, sizeof(end), hipMemcpyHostToDevice, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    exchange_sets(h, true);
    h->host_of.swap(host_of); h->h_point.swap(h_point); h->h_target.swap(h_target);
    h->n = n2; h->m = m2; h->linearized = false;                // eds_win_apply is EDS_ERR_STATE until the next eds_win_linearize
    if (h->wfl) h->wfl->fates_current = false;
    h->max_host = h->max_target = -1;
    for (int32_t v : h->host_of) if (v > h->max_host) h->max_host = v;
    for (int32_t v : h->h_target) if (v > h->max_target) h->max_target = v;
    if (inserted_points_out) *inserted_points_out = K;
    if (inserted_residuals_out) *inserted_residuals_out = R;
    return EDS_OK;
}

int eds_wed_counts(eds_win* h, int32_t* n, int32_t* m, int32_t* per_host) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (n) *n = h->n;
    if (m) *m = h->m;
    if (per_host) edswed::per_host_counts(h->host_of, per_host);
    return EDS_OK;
}

int eds_wed_get(eds_win* h, const eds_wed_out* o) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!o) return fail(EDS_ERR_INVALID, "null output");
    if (o->idepth_backup && !h->wsv) return fail(EDS_ERR_STATE, "eds_wed_get: no eds_wsv state was ever set, so there is no idepth backup");
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    hipStream_t st = h->own.st;
    std::vector<edswin::Point> p(o->host || o->uv || o->color || o->weights ? n : 0);
#define WED_GET(dst, src, count) if (o->dst && (count)) EDS_HIP_TRY(hipMemcpyAsync(o->dst, src, (count) * sizeof(*o->dst), hipMemcpyDeviceToHost, st))
    WED_GET(point, h->res_point, m);
    WED_GET(target, h->res_target, m);
    WED_GET(res_first, h->res_first, n + 1);
    WED_GET(idepth_zero_scaled, h->idz, n);
    WED_GET(deltaF, h->delta, n);
    if (o->idepth_backup && n && !h->wsv->have_backup) std::memset(o->idepth_backup, 0, n * sizeof(float));   // no backup holds: zeros
    else WED_GET(idepth_backup, h->wsv->backup, n);
#undef WED_GET
    if (!p.empty()) EDS_HIP_TRY(hipMemcpyAsync(p.data(), h->pts, n * sizeof(edswin::Point), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < p.size(); ++i) {
        if (o->host) o->host[i] = p[i].host;
        if (o->uv) { o->uv[2 * i] = p[i].u; o->uv[2 * i + 1] = p[i].v; }
        if (o->color) std::memcpy(o->color + 8 * i, p[i].color, 8 * sizeof(float));
        if (o->weights) std::memcpy(o->weights + 8 * i, p[i].weights, 8 * sizeof(float));
    }
    return EDS_OK;
}

}  // extern "C"
