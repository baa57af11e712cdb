// include/eds_hip_winflag.h: each point's residual history on the device.  The rules are eds_winflag.hpp, shared with the host; this
// file holds the kernels and the C entry points; the columns' journey through the edits is eds_winedit.hip's.  Everything of one call
// runs in the window's stream, in order.  Built without contraction into FMAs (csrc/Makefile): rel_baseline rounds as the host does.
//
// k_wfl_apply_fixed gives a point ONE lane that walks its run: a run is at most 7 residuals (one per other frame), each costs two
// dozen flops and five loads, and the point's updates (the maximum, the count, the two last states) have one order by construction.
// Eight lanes with a fold would save nothing at that length and would need the fold's order stated; the counts of the new states are
// integers, folded per wavefront and added with one integer atomic per wavefront and state.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_device.h"
#include "../../include/eds_hip_winflag.h"
#include "eds_capi_internal.hpp"
#include "eds_window_internal.hpp"
#include "eds_winedit.hpp"
#include "eds_winflag.hpp"

using edscapi::blocks;
using edscapi::fail;
using edswfl::Hist;

static_assert(edswfl::ST_IN == edswin::ST_IN && edswfl::ST_OOB == edswin::ST_OOB && edswfl::ST_OUTLIER == edswin::ST_OUTLIER, "eds_window.hpp's states");
static_assert(edswfl::PRECALC_FLOATS * sizeof(float) == sizeof(edswin::Precalc), "one precalc record");

namespace {

constexpr int TB = 256;
enum { COL_NUM_GOOD = 1, COL_MAX_REL = 2, COL_LAST_TARGET = 4, COL_LAST_STATE = 8, COL_IS_NEW = 16, COL_ALL = 31 };

// the defaults of the columns in `cols`, over n points and m residuals
__global__ void __launch_bounds__(TB) k_wfl_defaults(Hist h, int n, int m, int cols) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < n) {
        if (cols & COL_NUM_GOOD) h.num_good[i] = 0;
        if (cols & COL_MAX_REL) h.max_rel_baseline[i] = 0.0f;
        if (cols & COL_LAST_TARGET) h.last_target[2 * i] = h.last_target[2 * i + 1] = -1;
        if (cols & COL_LAST_STATE) h.last_state[2 * i] = h.last_state[2 * i + 1] = edswfl::ST_OOB;
    }
    if (i < m && (cols & COL_IS_NEW)) h.is_new[i] = 1;
}

__global__ void __launch_bounds__(TB) k_wfl_need(int n, int frame, const edswin::Point* __restrict__ pts, const int32_t* __restrict__ res_first,
                                                 const int32_t* __restrict__ res_target, int32_t* __restrict__ need) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n) need[p] = edswfl::needs_residual(res_first, res_target, pts[p].host, p, frame);
}
// the window's own residuals: where they go (map new -> old) and their point; every point's new first residual, the table's end too
__global__ void __launch_bounds__(TB) k_wfl_ins_old(int n, int m, const int32_t* __restrict__ res_first, const int32_t* __restrict__ res_point,
                                                    const int32_t* __restrict__ excl, int32_t* __restrict__ map_r, int32_t* __restrict__ res_point_new,
                                                    int32_t* __restrict__ res_first_new) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < m) {
        const int p = res_point[i], r = edswfl::moved_row(excl, p, i);
        map_r[r] = i;                                           // r < m + excl[n]: inside the new table
        res_point_new[r] = p;
    }
    if (i <= n) res_first_new[i] = edswfl::moved_first(res_first, excl, i);
}
// the new residuals, into the second set after the gather zeroed their rows: as eds_win_set_residuals leaves state IN and energy 0
__global__ void __launch_bounds__(TB) k_wfl_ins_new(int n, int frame, const int32_t* __restrict__ need, const int32_t* __restrict__ res_first,
                                                    const int32_t* __restrict__ excl, int32_t* __restrict__ res_point_new, int32_t* __restrict__ res_target_new,
                                                    int32_t* __restrict__ new_state_new, int32_t* __restrict__ is_new_new, Hist h) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= n || !need[p]) return;
    const int r = edswfl::new_row(res_first, excl, p);
    res_point_new[r] = p;
    res_target_new[r] = frame;
    new_state_new[r] = edswfl::ST_OUTLIER;
    is_new_new[r] = 1;
    edswfl::shift_last(h, p, frame);
}

// ---- eds_wfl_flag_points ------------------------------------------------------------------------------------------------------------------
// phase one, one lane per point walking its run (at most 7 residuals, three words each): the fate, and the mask of the candidates
__global__ void __launch_bounds__(TB) k_wfl_first_fate(int n, edswfl::Params prm, Hist h, const edswin::Point* __restrict__ pts, const float* __restrict__ ids,
                                                       const int32_t* __restrict__ res_first, const int32_t* __restrict__ res_target,
                                                       const int32_t* __restrict__ state, uint32_t frames_to_marg, int only_empty, int32_t* __restrict__ fate,
                                                       int32_t* __restrict__ mask) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const int32_t f = edswfl::first_fate(prm, h, p, pts[p].host, ids[p], res_first, res_target, state, frames_to_marg, only_empty);
    fate[p] = f;
    mask[p] = f == edswfl::CANDIDATE;
}
// phase two's first step for every residual of a candidate: resetOOB, and isLinearized = false (nothing in between reads it)
__global__ void __launch_bounds__(TB) k_wfl_reset(int m, const int32_t* __restrict__ mask, const int32_t* __restrict__ res_point, int32_t* __restrict__ state,
                                                  int32_t* __restrict__ new_state, float* __restrict__ energy, float* __restrict__ new_energy,
                                                  int32_t* __restrict__ lin) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m && mask[res_point[r]]) edswfl::reset_oob(r, state, new_state, energy, new_energy, lin);
}
// fixLinearizationF's selection: the residuals of the candidates that applyRes left active
__global__ void __launch_bounds__(TB) k_wfl_fix_select(int m, const int32_t* __restrict__ mask, const int32_t* __restrict__ res_point,
                                                       const int32_t* __restrict__ active, int32_t* __restrict__ sel) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r < m) sel[r] = mask[res_point[r]] && active[r];
}
// the candidates' fate from the Hessian; the totals (counts[0 .. 2]) and the same three per host frame (counts[3 + 3 host + fate]): integer atomics
__global__ void __launch_bounds__(TB) k_wfl_finish(int n, edswfl::Params prm, const edswin::Point* __restrict__ pts, const edswin::PointOut* __restrict__ pout,
                                                   int32_t* __restrict__ fate, int32_t* __restrict__ counts) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const int32_t f = edswfl::finish_fate(prm, fate[p], pout[p].idepth_hessian);
    fate[p] = f;
    atomicAdd(counts + f, 1);
    atomicAdd(counts + 3 + 3 * pts[p].host + f, 1);
}
// a per-point selection from the fates: fate == value, or (value < 0) fate != KEEP
__global__ void __launch_bounds__(TB) k_wfl_select(int n, const int32_t* __restrict__ fate, int value, int32_t* __restrict__ sel) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p < n) sel[p] = value < 0 ? fate[p] != edswfl::KEEP : fate[p] == value;
}

__global__ void __launch_bounds__(TB) k_wfl_apply_fixed(Hist h, int n, int F, const edswin::Precalc* __restrict__ pcs, const edswin::Point* __restrict__ pts,
                                                        const float* __restrict__ ids, const int32_t* __restrict__ res_first,
                                                        const int32_t* __restrict__ res_target, const int32_t* __restrict__ state,
                                                        const int32_t* __restrict__ active, int clear_is_new, int32_t* __restrict__ counts) {
    const int p = blockIdx.x * TB + threadIdx.x;
    int32_t c[3] = {0, 0, 0};
    if (p < n) {
        const edswin::Point* pt = pts + p;
        edswfl::apply_fixed_point(h, p, res_first, res_target, state, active, reinterpret_cast<const float*>(pcs), F, pt->host, pt->u, pt->v, ids[p], clear_is_new, c);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int total = edsdso::wave_fold_i(c[k]);
        if ((threadIdx.x & 63) == 0 && total) atomicAdd(counts + k, total);
    }
}

Hist first_set(const eds_wfl_state* f) { const Hist h = {f->num_good, f->max_rel_baseline, f->last_target, f->last_state, f->is_new}; return h; }

int queue_defaults(eds_win* h, int cols) {
    const int n = h->max_points, m = h->max_residuals, most = n > m ? n : m;
    hipLaunchKernelGGL(k_wfl_defaults, dim3(blocks(most)), dim3(TB), 0, h->own.st, first_set(h->wfl), n, m, cols);
    EDS_HIP_TRY(hipGetLastError());
    return EDS_OK;
}

// the columns, both sets, at the first call: the defaults over the whole capacity
int ensure_state(eds_win* h) {
    if (h->wfl) return EDS_OK;
    const size_t mp = (size_t)h->max_points, mr = (size_t)h->max_residuals;
    eds_wfl_state* f = new eds_wfl_state;
    const bool ok = h->own.alloc({{(void**)&f->num_good, mp * sizeof(int32_t)},
                                  {(void**)&f->max_rel_baseline, mp * sizeof(float)},
                                  {(void**)&f->last_target, mp * 2 * sizeof(int32_t)},
                                  {(void**)&f->last_state, mp * 2 * sizeof(int32_t)},
                                  {(void**)&f->is_new, mr * sizeof(int32_t)},
                                  {(void**)&f->num_good2, mp * sizeof(int32_t)},
                                  {(void**)&f->max_rel_baseline2, mp * sizeof(float)},
                                  {(void**)&f->last_target2, mp * 2 * sizeof(int32_t)},
                                  {(void**)&f->last_state2, mp * 2 * sizeof(int32_t)},
                                  {(void**)&f->is_new2, mr * sizeof(int32_t)},
                                  {(void**)&f->fate, mp * sizeof(int32_t)},
                                  {(void**)&f->mask, mp * sizeof(int32_t)},
                                  {(void**)&f->counts, 32 * sizeof(int32_t)}});
    if (!ok) {
        delete f;
        return fail(EDS_ERR_HIP, "eds_wfl: the device refused an allocation for the history columns");
    }
    h->wfl = f;
    if (int rc = queue_defaults(h, COL_ALL)) return rc;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

}  // namespace

namespace edswin_internal {

void wfl_release(eds_win* h) {
    delete h->wfl;
    h->wfl = nullptr;
}

int wfl_reset(eds_win* h) {
    if (!h->wfl) return EDS_OK;
    h->wfl->fates_current = false;
    if (int rc = queue_defaults(h, COL_ALL)) return rc;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

}  // namespace edswin_internal

extern "C" {

int eds_wfl_abi_version(void) { return EDS_HIP_WINFLAG_ABI_VERSION; }

int eds_wfl_set_history(eds_win* h, const eds_wfl_history* hist, int on_device) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    const eds_wfl_history none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const eds_wfl_history& a = hist ? *hist : none;
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    const struct { const void* src; size_t words; int col; } cols[5] = {{a.num_good, n, COL_NUM_GOOD}, {a.max_rel_baseline, n, COL_MAX_REL},
                                                                         {a.last_target, 2 * n, COL_LAST_TARGET}, {a.last_state, 2 * n, COL_LAST_STATE},
                                                                         {a.is_new, m, COL_IS_NEW}};
    for (const auto& c : cols)
        if (on_device && c.src && c.words)
            if (int rc = eds_dev_check_range(h->own.dev, c.src, c.words * 4)) return rc;
    if (!on_device) {
        for (size_t i = 0; a.last_target && i < 2 * n; ++i)
            if (a.last_target[i] < -1 || a.last_target[i] >= EDS_WIN_MAX_FRAMES) return fail(EDS_ERR_INVALID, "eds_wfl_set_history: last_target is -1 .. 7");
        for (size_t i = 0; a.last_state && i < 2 * n; ++i)
            if (a.last_state[i] < 0 || a.last_state[i] > 2) return fail(EDS_ERR_INVALID, "eds_wfl_set_history: last_state is 0 IN, 1 OOB or 2 OUTLIER");
    }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    eds_wfl_state* f = h->wfl;
    void* const dst[5] = {f->num_good, f->max_rel_baseline, f->last_target, f->last_state, f->is_new};
    int defaults = 0;
    for (int k = 0; k < 5; ++k) {
        if (!cols[k].src) defaults |= cols[k].col;
        else if (cols[k].words)
            EDS_HIP_TRY(hipMemcpyAsync(dst[k], cols[k].src, cols[k].words * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->own.st));
    }
    if (defaults)
        if (int rc = queue_defaults(h, defaults)) return rc;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_wfl_get_history(eds_win* h, const eds_wfl_history* o) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!o) return fail(EDS_ERR_INVALID, "null output");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    const eds_wfl_state* f = h->wfl;
    const size_t n = (size_t)h->n, m = (size_t)h->m;
    hipStream_t st = h->own.st;
#define WFL_GET(dst, src, count) if (o->dst && (count)) EDS_HIP_TRY(hipMemcpyAsync(o->dst, src, (count) * 4, hipMemcpyDeviceToHost, st))
    WFL_GET(num_good, f->num_good, n);
    WFL_GET(max_rel_baseline, f->max_rel_baseline, n);
    WFL_GET(last_target, f->last_target, 2 * n);
    WFL_GET(last_state, f->last_state, 2 * n);
    WFL_GET(is_new, f->is_new, m);
#undef WFL_GET
    EDS_HIP_TRY(hipStreamSynchronize(st));
    return EDS_OK;
}

int eds_wfl_insert_frame_residuals(eds_win* h, int frame, int32_t* inserted_out) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (frame < 0 || frame >= h->max_frames) return fail(EDS_ERR_INVALID, "frame " + std::to_string(frame) + " outside the handle's");
    const int n = h->n, m = h->m;
    // the host's copies say what will be inserted: a refusal queues nothing
    std::vector<int32_t> need((size_t)n, 0), excl((size_t)n + 1, 0);
    for (int p = 0; p < n; ++p) need[p] = h->host_of[p] != frame;
    for (int r = 0; r < m; ++r) if (h->h_target[r] == frame) need[h->h_point[r]] = 0;
    int K = 0;
    for (int p = 0; p < n; ++p) { excl[p] = K; K += need[p]; }
    excl[n] = K;
    const int m2 = m + K;
    if (m2 > h->max_residuals)
        return fail(EDS_ERR_STATE, "eds_wfl_insert_frame_residuals: " + std::to_string(m2) + " residuals do not fit the window's " + std::to_string(h->max_residuals));
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    if (int rc = edswin_internal::wed_ensure_state(h)) return rc;
    if (inserted_out) *inserted_out = K;
    if (!K) { h->linearized = false; return EDS_OK; }
    eds_wed_state* s = h->wed;
    eds_wfl_state* f = h->wfl;
    hipStream_t st = h->own.st;
    // the flags and their exclusive sums on the device, by winedit's scan; the flags come back for the check against the host's copies
    hipLaunchKernelGGL(k_wfl_need, dim3(blocks(n)), dim3(TB), 0, st, n, frame, h->pts, h->res_first, h->res_target, s->keep_p);
    if (int rc = edswin_internal::wed_queue_scan(h, s->keep_p, n, s->excl_p, s->map_p, s->total)) return rc;
    std::vector<int32_t> flags((size_t)n);
    int32_t total = 0;
    EDS_HIP_TRY(hipMemcpyAsync(flags.data(), s->keep_p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipMemcpyAsync(&total, s->total, sizeof(total), hipMemcpyDeviceToHost, st));
    EDS_HIP_TRY(hipStreamSynchronize(st));
    if (total != K || flags != need)
        return fail(EDS_ERR_HIP, "eds_wfl_insert_frame_residuals: the device's flags and the host's copies of the tables differ");
    // the tables: old rows to their new places (map new -> old, -1 for a new row: the gather zeroes it), then the new rows' own values
    EDS_HIP_TRY(hipMemsetAsync(s->map_r, 0xff, (size_t)m2 * sizeof(int32_t), st));
    const int most = n + 1 > m ? n + 1 : m;
    hipLaunchKernelGGL(k_wfl_ins_old, dim3(blocks(most)), dim3(TB), 0, st, n, m, h->res_first, h->res_point, s->excl_p, s->map_r, s->res_point, s->res_first);
    edswin_internal::wed_queue_residual_rows(h, s->map_r, m2);
    hipLaunchKernelGGL(k_wfl_ins_new, dim3(blocks(n)), dim3(TB), 0, st, n, frame, s->keep_p, h->res_first, s->excl_p, s->res_point, s->res_target, s->new_state,
                       f->is_new2, first_set(f));
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(st));
    edswin_internal::wed_exchange_residual_sets(h);
    // the host's copies, from the same flags
    std::vector<int32_t> h_point((size_t)m2), h_target((size_t)m2);
    for (int r = 0; r < m; ++r) {
        const int i = edswfl::moved_row(excl.data(), h->h_point[r], r);
        h_point[i] = h->h_point[r]; h_target[i] = h->h_target[r];
    }
    std::vector<int32_t> res_first((size_t)n + 1, 0);
    for (int r = 0; r < m; ++r) ++res_first[h->h_point[r] + 1];
    for (int p = 0; p < n; ++p) res_first[p + 1] += res_first[p];
    for (int p = 0; p < n; ++p)
        if (need[p]) {
            const int i = edswfl::new_row(res_first.data(), excl.data(), p);
            h_point[i] = p; h_target[i] = frame;
        }
    h->h_point.swap(h_point); h->h_target.swap(h_target);
    h->m = m2; h->linearized = false;
    f->fates_current = false;
    if (frame > h->max_target) h->max_target = frame;
    return EDS_OK;
}

int eds_wfl_apply_fixed(eds_win* h, int F, const float* precalc, int clear_is_new, int32_t* counts) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (F < 2 || F > h->max_frames) return fail(EDS_ERR_INVALID, "F is 2 .. max_frames");
    if (clear_is_new != 0 && clear_is_new != 1) return fail(EDS_ERR_INVALID, "clear_is_new is 0 or 1");
    if (!precalc) return fail(EDS_ERR_INVALID, "precalc is required");
    if (h->max_host >= F || h->max_target >= F) return fail(EDS_ERR_INVALID, "a point's host or a residual's target is not below F");
    for (size_t i = 0; i < (size_t)F * F * edswfl::PRECALC_FLOATS; ++i)
        if (!std::isfinite(precalc[i])) return fail(EDS_ERR_INVALID, "precalc is not finite");
    if (!h->linearized) return fail(EDS_ERR_STATE, "eds_wfl_apply_fixed before eds_win_linearize");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    eds_wfl_state* f = h->wfl;
    hipStream_t st = h->own.st;
    int32_t back[4] = {0, 0, 0, 0};
    if (h->n) {
        EDS_HIP_TRY(hipMemcpyAsync(h->pcs, precalc, (size_t)F * F * sizeof(edswin::Precalc), hipMemcpyHostToDevice, st));
        EDS_HIP_TRY(hipMemsetAsync(f->counts, 0, 4 * sizeof(int32_t), st));
        edswin_internal::queue_apply(h, 1, nullptr);
        hipLaunchKernelGGL(k_wfl_apply_fixed, dim3(blocks(h->n)), dim3(TB), 0, st, first_set(f), h->n, F, h->pcs, h->pts, h->ids, h->res_first, h->res_target, h->state,
                           h->active, clear_is_new, f->counts);
        EDS_HIP_TRY(hipGetLastError());
        EDS_HIP_TRY(hipMemcpyAsync(back, f->counts, sizeof(back), hipMemcpyDeviceToHost, st));
        EDS_HIP_TRY(hipStreamSynchronize(st));                 // precalc may be pageable
    }
    if (counts) for (int k = 0; k < 3; ++k) counts[k] = back[k];
    return EDS_OK;
}

void eds_wfl_params_default(eds_wfl_params* p) {
    if (!p) return;
    const edswfl::Params d = edswfl::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_wfl_flag_points(eds_win* h, int F, uint32_t frames_to_marg, const eds_wfl_params* params, const float* precalc, const float* frame_energy_th,
                        int only_empty, int32_t* counts) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (F < 2 || F > h->max_frames) return fail(EDS_ERR_INVALID, "F is 2 .. max_frames");
    if (only_empty != 0 && only_empty != 1) return fail(EDS_ERR_INVALID, "only_empty is 0 or 1");
    if (!params || !precalc || !frame_energy_th) return fail(EDS_ERR_INVALID, "params, precalc and frame_energy_th are required");
    if (frames_to_marg >> F) return fail(EDS_ERR_INVALID, "frames_to_marg names a frame that is not below F");
    edswfl::Params prm;
    std::memcpy(&prm, params, sizeof(prm));
    if (!std::isfinite(prm.min_idepth_h_marg)) return fail(EDS_ERR_INVALID, "min_idepth_h_marg is not finite");
    if (h->max_host >= F || h->max_target >= F) return fail(EDS_ERR_INVALID, "a point's host or a residual's target is not below F");
    for (size_t i = 0; i < (size_t)F * F * edswfl::PRECALC_FLOATS; ++i)
        if (!std::isfinite(precalc[i])) return fail(EDS_ERR_INVALID, "precalc is not finite");
    for (int f = 0; f < F; ++f)
        if (!std::isfinite(frame_energy_th[f])) return fail(EDS_ERR_INVALID, "frame_energy_th is not finite");
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_win: no calibration set");
    for (int f = 0; f < F; ++f)
        if (!(h->frames_set >> f & 1u)) return fail(EDS_ERR_STATE, "eds_win: frame " + std::to_string(f) + " was never set");
    if (!h->wsv || !h->wsv->valid) return fail(EDS_ERR_STATE, "eds_wfl_flag_points: no eds_wsv state set (fixLinearizationF reads it)");
    if (h->wsv->F != F) return fail(EDS_ERR_INVALID, "eds_wfl_flag_points: F is not the eds_wsv state's");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = ensure_state(h)) return rc;
    eds_wfl_state* f = h->wfl;
    eds_wsv_state* v = h->wsv;
    hipStream_t st = h->own.st;
    int32_t back[27];
    std::memset(back, 0, sizeof(back));
    f->fates_current = false;
    if (h->n) {
        const int n = h->n, m = h->m;
        EDS_HIP_TRY(hipMemcpyAsync(h->pcs, precalc, (size_t)F * F * sizeof(edswin::Precalc), hipMemcpyHostToDevice, st));
        EDS_HIP_TRY(hipMemcpyAsync(h->th, frame_energy_th, (size_t)F * sizeof(float), hipMemcpyHostToDevice, st));
        EDS_HIP_TRY(hipMemsetAsync(f->counts, 0, 32 * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_wfl_first_fate, dim3(blocks(n)), dim3(TB), 0, st, n, prm, first_set(f), h->pts, h->ids, h->res_first, h->res_target, h->state,
                           frames_to_marg, only_empty, f->fate, f->mask);
        if (m && !only_empty) {                                 // the bodies of eds_win_linearize, eds_win_apply and eds_wsv_fix_linearization behind the mask
            hipLaunchKernelGGL(k_wfl_reset, dim3(blocks(m)), dim3(TB), 0, st, m, f->mask, h->res_point, h->state, h->new_state, h->energy, h->new_energy, v->lin);
            edswin_internal::queue_linearize(h, F, f->mask);
            edswin_internal::queue_apply(h, 1, f->mask);
            hipLaunchKernelGGL(k_wfl_fix_select, dim3(blocks(m)), dim3(TB), 0, st, m, f->mask, h->res_point, h->active, v->sel);
            edswin_internal::wsv_queue_fix(h, v->sel);
        }
        hipLaunchKernelGGL(k_wfl_finish, dim3(blocks(n)), dim3(TB), 0, st, n, prm, h->pts, h->pout, f->fate, f->counts);
        EDS_HIP_TRY(hipGetLastError());
        EDS_HIP_TRY(hipMemcpyAsync(back, f->counts, sizeof(back), hipMemcpyDeviceToHost, st));
        EDS_HIP_TRY(hipStreamSynchronize(st));
    }
    f->fates_current = true;
    if (counts) std::memcpy(counts, back, sizeof(back));
    return EDS_OK;
}

int eds_wfl_get_fates(eds_win* h, int32_t* fate) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!fate && h->n) return fail(EDS_ERR_INVALID, "null output");
    if (!h->wfl || !h->wfl->fates_current) return fail(EDS_ERR_STATE, "eds_wfl: no fates are current (eds_wfl_flag_points; every edit of the tables makes them stale)");
    return edscapi::read_back(h->own, fate, h->wfl->fate, (size_t)h->n * sizeof(int32_t));
}

int eds_wfl_marginalize_flagged(eds_win* h, float prior_fac, double weight_fac, double* HM, double* bM, int32_t* res_in_m) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!h->wfl || !h->wfl->fates_current) return fail(EDS_ERR_STATE, "eds_wfl: no fates are current (eds_wfl_flag_points; every edit of the tables makes them stale)");
    if (!h->wsv || !h->wsv->valid) return fail(EDS_ERR_STATE, "eds_wfl_marginalize_flagged: no eds_wsv state set");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (h->n) hipLaunchKernelGGL(k_wfl_select, dim3(blocks(h->n)), dim3(TB), 0, h->own.st, h->n, h->wfl->fate, (int)edswfl::MARGINALIZE, h->wsv->sel);
    EDS_HIP_TRY(hipGetLastError());
    return edswin_internal::wsv_marginalize_points(h, nullptr, prior_fac, weight_fac, HM, bM, res_in_m);      // the upload skipped: the flags are there
}

int eds_wfl_remove_flagged(eds_win* h, int32_t* points_gone, int32_t* residuals_gone) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!h->wfl || !h->wfl->fates_current) return fail(EDS_ERR_STATE, "eds_wfl: no fates are current (eds_wfl_flag_points; every edit of the tables makes them stale)");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (h->n) hipLaunchKernelGGL(k_wfl_select, dim3(blocks(h->n)), dim3(TB), 0, h->own.st, h->n, h->wfl->fate, -1, h->wfl->mask);
    EDS_HIP_TRY(hipGetLastError());
    return eds_wed_remove_points(h, h->wfl->mask, 1, points_gone, residuals_gone);
}

}  // extern "C"
