// include/eds_hip_init.h: DSO's CoarseInitializer on the device.  The arithmetic and the whole of trackFrame are eds_init.hpp, shared with
// the host; this file holds the evaluator that runs it in one workgroup, three kernels and the C entry points.  Built without contraction
// into FMAs (csrc/Makefile).
//
// k_ini_track runs trackFrame for one new frame in ONE workgroup of 512 lanes: the lanes stride a level's points (a point per lane), keep
// fp64 partials and fold them in eds_coarse.hpp's order; lane 0 alone assembles the 8 x 8 systems, solves and steps the pose in LDS, and
// every lane reads the uniform results after a barrier.  The order-dependent loops run one barrier per depth of the level's schedule.
// Every loop is bounded by max_iterations, the fails counter or a table's size, and no workgroup waits on another: nothing can spin.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_init.h"
#include "eds_capi_internal.hpp"
#include "eds_init.hpp"
#include "eds_init_internal.hpp"
#include "eds_pixsel_internal.hpp"

using edscapi::fail;
using edsct::Geo;
using edsct::Level;
using edsdso::Px;
using edsini::Carry;
using edsini::Frame;
using edsini::Lv;
using edsini::Params;
using edsini::Pnt;
using edsini::Result;

static_assert(sizeof(Params) == sizeof(eds_ini_params), "edsini::Params is eds_ini_params member for member");
static_assert(sizeof(Result) == sizeof(eds_ini_result), "edsini::Result is eds_ini_result member for member");
static_assert(sizeof(Pnt) == 64 && sizeof(Pnt) == sizeof(eds_ini_point), "one point is 16 words");
static_assert(edsini::MAX_DECISIONS == EDS_INI_MAX_DECISIONS && edsini::MAX_LEVELS == EDS_INI_MAX_LEVELS && edsini::NN == EDS_INI_NEIGHBOURS &&
                  edsini::MAX_ITERATIONS == EDS_INI_MAX_ITERATIONS,
              "header constants");

// struct eds_ini is eds_init_internal.hpp's, shared with eds_inisetup.hip.  Its device memory has one owner, the member
// `edscapi::DeviceOwner own;`: this file allocates and frees through it alone.

namespace {

using edsdso::LANES;

// the evaluator of eds_init.hpp's templates on the device
struct DevEv {
    double* part;                                          // LDS: [46][8]
    __device__ bool writer() const { return threadIdx.x == 0; }
    __device__ void sync() { __syncthreads(); }
    template <class F> __device__ void each(int n, F f) {
        for (int i = threadIdx.x; i < n; i += LANES) f(i);
        __syncthreads();
    }
    // one barrier per depth.  A lane's record of the NEXT depth and the bound after it are fetched before the barrier (the schedule is
    // read-only), so what a step waits for after the barrier is only what other points wrote.
    template <class F> __device__ void each_sched(const int32_t* sched, const int32_t* doff, int nd, F f) {
        if (nd <= 0) return;
        const int4* rows = reinterpret_cast<const int4*>(sched);
        int hi = doff[1], k = doff[0] + (int)threadIdx.x;
        bool have = k < hi;
        int4 r[3] = {make_int4(0, -1, -1, -1), make_int4(-1, -1, -1, -1), make_int4(-1, -1, -1, 0)};
        if (have) { r[0] = rows[3 * (size_t)k]; r[1] = rows[3 * (size_t)k + 1]; r[2] = rows[3 * (size_t)k + 2]; }
        for (int d = 0; d < nd; ++d) {
            const int hi2 = d + 2 <= nd ? doff[d + 2] : hi;
            if (have) {
                const int32_t rec[edsini::SCHED] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w};
                f(rec[0], rec + 1);
            }
            for (int k2 = k + LANES; k2 < hi; k2 += LANES) {             // a depth of more than 512 points
                const int4 a = rows[3 * (size_t)k2], b = rows[3 * (size_t)k2 + 1], c = rows[3 * (size_t)k2 + 2];
                const int32_t rec[edsini::SCHED] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
                f(rec[0], rec + 1);
            }
            k = hi + (int)threadIdx.x;
            hi = hi2;
            have = d + 1 < nd && k < hi;
            if (have) { r[0] = rows[3 * (size_t)k]; r[1] = rows[3 * (size_t)k + 1]; r[2] = rows[3 * (size_t)k + 2]; }
            __syncthreads();
        }
    }
    template <int NQ, class F> __device__ void reduce(int n, double* S, F f) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
        for (int i = threadIdx.x; i < n; i += LANES) f(i, acc);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double v = edsdso::wave_fold(acc[q]);
            if (lane == 0) part[8 * q + wave] = v;
        }
        __syncthreads();
        if ((int)threadIdx.x < NQ) {
            S[threadIdx.x] = edsdso::add8(part + 8 * threadIdx.x);
        }
        __syncthreads();
    }
};

__global__ void __launch_bounds__(LANES) k_ini_pyramid(Geo g, const float* __restrict__ img, Px* __restrict__ px) {
    DevEv ev;
    ev.part = nullptr;
    edsini::build_pyramid(ev, g, img, px);
}

// one level's points: the rectangle in row-major order, 512 pixels a trip; a selected pixel's place is the count before its trip plus
// its rank in the trip (block_rank).  Places past `cap` are counted and not written.
template <class T>
__global__ void __launch_bounds__(LANES) k_ini_points(const T* __restrict__ status, int w, int h, Params s, Pnt* __restrict__ out, int cap,
                                                      int32_t* __restrict__ count) {
    __shared__ int s_wave[LANES / 64];
    int base = 0;
    for (int start = 0; start < w * h; start += LANES) {
        const int i = start + threadIdx.x, x = i % w, y = i / w;
        const bool sel = i < w * h && edsini::in_rect(x, y, w, h) && status[i] != 0;
        int total;
        const int at = base + edsdso::block_rank<LANES>(sel, s_wave, &total);
        if (sel && at < cap) out[at] = edsini::make_point(x, y, (float)status[i], s);
        base += total;
    }
    if (threadIdx.x == 0) *count = base;
}

__global__ void __launch_bounds__(LANES) k_ini_track(Frame f, Carry* carry, Result* out) {
    __shared__ edsini::Shared sh;
    __shared__ double part[46 * 8];
    DevEv ev;
    ev.part = part;
    edsini::track_frame(ev, f, &sh, carry, out);
}

// Every kernel launch and every wait of this file goes through these three, which count on the handle: eds_ini_result.launches / .waits
// are the counters' differences over one eds_ini_track_frame, so a launch or a wait added anywhere in that call shows.
#define INI_LAUNCH(h, kernel, ...)                                                                  \
    do {                                                                                            \
        hipLaunchKernelGGL(kernel, dim3(1), dim3(LANES), 0, (h)->own.st, __VA_ARGS__);              \
        ++(h)->n_launches;                                                                          \
    } while (0)

int ini_wait(eds_ini* h) {
    ++h->n_waits;
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int ini_read_back(eds_ini* h, void* dst, const void* src, size_t bytes) {
    if (dst && bytes) ++h->n_waits;
    return edscapi::read_back(h->own, dst, src, bytes);
}

int check_level(const eds_ini* h, int lvl) {
    if (lvl < 0 || lvl >= h->geo.levels) return fail(EDS_ERR_INVALID, "level " + std::to_string(lvl) + " outside 0 .. " + std::to_string(h->geo.levels - 1));
    return EDS_OK;
}

int upload_carry(eds_ini* h) {
    EDS_HIP_TRY(hipMemcpyAsync(h->d_carry, &h->carry, sizeof(Carry), hipMemcpyHostToDevice, h->own.st));
    return ini_wait(h);
}

// after k_ini_points: the count comes back as one integer; the level's buffers start from zero
int finish_points(eds_ini* h, int lvl, int32_t* n_out) {
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipMemsetAsync(h->jb + (size_t)lvl * 2 * h->cap * 10, 0, (size_t)2 * h->cap * 10 * sizeof(float), h->own.st));
    int32_t n = 0;
    if (int rc = ini_read_back(h, &n, h->d_count, sizeof(n))) return rc;
    h->points_set[lvl] = false;
    h->tables_set[lvl] = false;
    h->nn_made[lvl] = false;
    if (lvl > 0) h->tables_set[lvl - 1] = h->nn_made[lvl - 1] = false;
    if (n > h->cap) return fail(EDS_ERR_INVALID, std::to_string(n) + " selected pixels, the handle holds " + std::to_string(h->cap) + " per level");
    h->n[lvl] = n;
    h->points_set[lvl] = true;
    if (n_out) *n_out = n;
    return EDS_OK;
}

}  // namespace

int edsini_internal::points_from_bytes(eds_ini* h, int lvl, const uint8_t* map, int32_t* n_out) {
    const Level& L = h->geo.l[lvl];
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    INI_LAUNCH(h, k_ini_points<uint8_t>, map, L.w, L.h, h->prm, h->pts + (size_t)lvl * h->cap, h->cap, h->d_count);
    return finish_points(h, lvl, n_out);
}

extern "C" {

int eds_ini_abi_version(void) { return EDS_HIP_INIT_ABI_VERSION; }

void eds_ini_params_default(eds_ini_params* p) {
    if (!p) return;
    const Params d = edsini::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_ini_create(int device, int H, int W, int levels, int max_points_per_level, eds_ini** ini) {
    if (!ini) return fail(EDS_ERR_INVALID, "null output");
    *ini = nullptr;
    if (!edsct::shape_valid(H, W, levels))
        return fail(EDS_ERR_INVALID, "levels are 1 .. 5, H and W 8 .. 8192 and divisible by 2^(levels - 1), the coarsest level at least 8 x 8");
    if (max_points_per_level < 1 || max_points_per_level > EDS_INI_MAX_POINTS) return fail(EDS_ERR_INVALID, "max_points_per_level is 1 .. 65536");
    eds_ini* h = new eds_ini;
    if (int rc = h->own.open(device)) { delete h; return rc; }
    h->cap = max_points_per_level;
    edsct::make_shape(h->geo, H, W, levels);
    h->prm = edsini::params_default();
    std::memset(&h->carry, 0, sizeof(h->carry));
    const size_t tot = (size_t)h->geo.total, px0 = (size_t)H * W, lc = (size_t)levels * h->cap;
    const bool ok = h->own.alloc({{(void**)&h->first_px, tot * sizeof(Px)},
                                  {(void**)&h->new_px, tot * sizeof(Px)},
                                  {(void**)&h->in_img, px0 * sizeof(float)},
                                  {(void**)&h->in_status, px0 * sizeof(float)},
                                  {(void**)&h->pts, lc * sizeof(Pnt)},
                                  {(void**)&h->sched, lc * edsini::SCHED * sizeof(int32_t)},
                                  {(void**)&h->parent, lc * sizeof(int32_t)},
                                  {(void**)&h->doff, (lc + levels) * sizeof(int32_t)},
                                  {(void**)&h->coff, (lc + levels) * sizeof(int32_t)},
                                  {(void**)&h->child, lc * sizeof(int32_t)},
                                  {(void**)&h->jb, lc * 2 * 10 * sizeof(float)},
                                  {(void**)&h->iR_old, (size_t)h->cap * sizeof(float)},
                                  {(void**)&h->good_old, (size_t)h->cap * sizeof(int32_t)},
                                  {(void**)&h->d_count, sizeof(int32_t)},
                                  {(void**)&h->d_carry, sizeof(Carry)},
                                  {(void**)&h->d_out, sizeof(Result)}});
    if (!ok || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        (void)hipGetLastError();
        eds_ini_destroy(h);
        return fail(EDS_ERR_HIP, "eds_ini_create: the device refused a stream or an allocation");
    }
    *ini = h;
    return EDS_OK;
}

void eds_ini_destroy(eds_ini* h) {
    if (!h) return;
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    h->own.close();
    delete h;
}

int eds_ini_set_params(eds_ini* h, const eds_ini_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null parameters");
    Params s;
    std::memcpy(&s, p, sizeof(s));
    if (!edsini::params_valid(s))
        return fail(EDS_ERR_INVALID, "parameters: every float finite; huber_th, outlier_th and the scales > 0; fix_affine 0 or 1; max_iterations 0 .. 100");
    h->prm = s;
    return EDS_OK;
}

int eds_ini_get_params(const eds_ini* h, eds_ini_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(p, &h->prm, sizeof(*p));
    return EDS_OK;
}

int eds_ini_set_calib(eds_ini* h, float fx, float fy, float cx, float cy) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!edscapi::check_calib(fx, fy, cx, cy)) return fail(EDS_ERR_INVALID, "calibration: fx, fy, cx, cy finite, fx and fy > 0");
    edsct::make_k(h->geo, fx, fy, cx, cy);
    h->calib_set = true;
    return EDS_OK;
}

int eds_ini_set_first(eds_ini* h, const float* image, int64_t row_stride, int on_device, float exposure) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_ini: no calibration set");
    if (!std::isfinite(exposure)) return fail(EDS_ERR_INVALID, "exposure must be finite");
    if (int rc = edscapi::check_images(h->own.dev, h->geo.H, h->geo.W, 1, image, &row_stride, nullptr, on_device, "image")) return rc;
    h->first_set = false;
    for (int l = 0; l < edsini::MAX_LEVELS; ++l) h->status_set[l] = false;      // include/eds_hip_inisetup.h: the maps were of the frame before
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edscapi::upload_image(h->own, h->in_img, h->geo.H, h->geo.W, image, row_stride, on_device)) return rc;
    INI_LAUNCH(h, k_ini_pyramid, h->geo, h->in_img, h->first_px);
    EDS_HIP_TRY(hipGetLastError());
    const double aff[2] = {h->carry.aff[0], h->carry.aff[1]};              // :766-768 leave thisToNext_aff as it is
    std::memset(&h->carry, 0, sizeof(h->carry));
    h->carry.T[0] = h->carry.T[5] = h->carry.T[10] = 1.0;
    h->carry.aff[0] = aff[0]; h->carry.aff[1] = aff[1];
    if (int rc = upload_carry(h)) return rc;
    h->exposure_first = exposure;
    h->first_set = true;
    h->new_set = false;
    return EDS_OK;
}

int eds_ini_set_pose(eds_ini* h, const double* T, const double* aff) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!T || !aff) return fail(EDS_ERR_INVALID, "T and aff are required");
    for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) return fail(EDS_ERR_INVALID, "T is not finite");
    if (!std::isfinite(aff[0]) || !std::isfinite(aff[1])) return fail(EDS_ERR_INVALID, "aff is not finite");
    if (!h->first_set) return fail(EDS_ERR_STATE, "eds_ini: no first frame set");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    Carry c = h->carry;
    std::memcpy(c.T, T, sizeof(c.T));
    c.aff[0] = aff[0]; c.aff[1] = aff[1];
    h->carry = c;
    return upload_carry(h);
}

int eds_ini_set_points(eds_ini* h, int lvl, const float* status, int64_t row_stride, int on_device, int32_t* n_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    const Level& L = h->geo.l[lvl];
    if (int rc = edscapi::check_images(h->own.dev, L.h, L.w, 1, status, &row_stride, nullptr, on_device, "status")) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edscapi::upload_image(h->own, h->in_status, L.h, L.w, status, row_stride, on_device)) return rc;
    INI_LAUNCH(h, k_ini_points<float>, h->in_status, L.w, L.h, h->prm, h->pts + (size_t)lvl * h->cap, h->cap, h->d_count);
    return finish_points(h, lvl, n_out);
}

int eds_ini_set_points_selected(eds_ini* h, eds_sel* sel, int32_t* n_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = edscapi::check_handle(sel, "eds_sel")) return rc;
    if (sel->H != h->geo.H || sel->W != h->geo.W || sel->own.dev != h->own.dev)
        return fail(EDS_ERR_INVALID, "the selector must be of the handle's H x W and on its device");
    if (!sel->sel_valid) return fail(EDS_ERR_STATE, "eds_sel: no selection holds (eds_sel_make_maps first)");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    INI_LAUNCH(h, k_ini_points<uint8_t>, sel->map, h->geo.W, h->geo.H, h->prm, h->pts, h->cap, h->d_count);
    return finish_points(h, 0, n_out);
}

int eds_ini_make_nn(int n, const float* uv, int n_up, const float* uv_up, int32_t* neighbours, int32_t* parent) {
    if (n < 0 || n_up < 0 || (n > 0 && (!uv || !neighbours))) return fail(EDS_ERR_INVALID, "uv and neighbours are required");
    if (parent && (n_up < 1 || !uv_up)) return fail(EDS_ERR_INVALID, "a parent table needs the points of the level above");
    for (int i = 0; i < 2 * n; ++i) if (!std::isfinite(uv[i])) return fail(EDS_ERR_INVALID, "uv is not finite");
    for (int i = 0; parent && i < 2 * n_up; ++i) if (!std::isfinite(uv_up[i])) return fail(EDS_ERR_INVALID, "uv_up is not finite");
    edsini::make_nn(n, uv, parent ? n_up : 0, uv_up, neighbours, parent);
    return EDS_OK;
}

int eds_ini_set_neighbours(eds_ini* h, int lvl, const int32_t* neighbours, const int32_t* parent) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    const bool top = lvl == h->geo.levels - 1;
    if (!neighbours || (!top && !parent)) return fail(EDS_ERR_INVALID, "neighbours (and, below the top level, parent) are required");
    if (!h->points_set[lvl] || (!top && !h->points_set[lvl + 1])) return fail(EDS_ERR_STATE, "eds_ini: the points of the level and of the level above come first");
    const int n = h->n[lvl], np = top ? 0 : h->n[lvl + 1];
    std::vector<int32_t> sched(((size_t)n + 1) * edsini::SCHED), doff((size_t)n + 2), coff((size_t)np + 2), child((size_t)n + 1);
    int32_t nd = 0;
    if (!edsini::derive_tables(n, neighbours, top ? nullptr : parent, np, sched.data(), doff.data(), &nd, coff.data(), child.data()))
        return fail(EDS_ERR_INVALID, "a neighbour is outside -1 .. n - 1 or a parent outside 0 .. n_up - 1");
    h->tables_set[lvl] = false;
    h->nn_made[lvl] = false;                                // eds_ini_make_neighbours sets it again after this call
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t o = (size_t)lvl * h->cap, o1 = (size_t)lvl * (h->cap + 1);
    if (n > 0) {
        EDS_HIP_TRY(hipMemcpyAsync(h->sched + o * edsini::SCHED, sched.data(), (size_t)n * edsini::SCHED * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
        if (!top) {
            EDS_HIP_TRY(hipMemcpyAsync(h->parent + o, parent, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
            EDS_HIP_TRY(hipMemcpyAsync(h->child + o, child.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
        }
    }
    EDS_HIP_TRY(hipMemcpyAsync(h->doff + o1, doff.data(), (size_t)(nd + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    if (!top) EDS_HIP_TRY(hipMemcpyAsync(h->coff + o1, coff.data(), (size_t)(np + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    if (int rc = ini_wait(h)) return rc;
    h->nd[lvl] = nd;
    h->tables_set[lvl] = true;
    return EDS_OK;
}

int eds_ini_get_schedule_depth(const eds_ini* h, int lvl, int32_t* depth_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (!depth_out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->tables_set[lvl]) return fail(EDS_ERR_STATE, "eds_ini: the level has no tables");
    *depth_out = h->nd[lvl];
    return EDS_OK;
}

int eds_ini_track_frame(eds_ini* h, const float* image, int64_t row_stride, int on_device, float exposure, int snapped_threshold,
                        eds_ini_result* out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!std::isfinite(exposure)) return fail(EDS_ERR_INVALID, "exposure must be finite");
    if (snapped_threshold < 0 || snapped_threshold > (1 << 20)) return fail(EDS_ERR_INVALID, "snapped_threshold is 0 .. 2^20");
    if (!h->first_set) return fail(EDS_ERR_STATE, "eds_ini: no first frame set");
    for (int l = 0; l < h->geo.levels; ++l)
        if (!h->points_set[l] || !h->tables_set[l]) return fail(EDS_ERR_STATE, "eds_ini: level " + std::to_string(l) + " has no points or no tables");
    if (int rc = edscapi::check_images(h->own.dev, h->geo.H, h->geo.W, 1, image, &row_stride, nullptr, on_device, "image")) return rc;
    const long launches0 = h->n_launches, waits0 = h->n_waits;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edscapi::upload_image(h->own, h->in_img, h->geo.H, h->geo.W, image, row_stride, on_device)) return rc;
    Frame f;
    std::memset(&f, 0, sizeof(f));
    f.g = h->geo; f.s = h->prm;
    for (int l = 0; l < h->geo.levels; ++l) {
        const size_t o = (size_t)l * h->cap, o1 = (size_t)l * (h->cap + 1);
        Lv& L = f.lv[l];
        L.p = h->pts + o; L.sched = h->sched + o * edsini::SCHED; L.parent = h->parent + o; L.doff = h->doff + o1;
        L.coff = h->coff + o1; L.child = h->child + o; L.jb = h->jb + o * 2 * 10;
        L.n = h->n[l]; L.nd = h->nd[l]; L.n_parents = l + 1 < h->geo.levels ? h->n[l + 1] : 0; L.cap = h->cap;
    }
    f.ref = h->first_px; f.nw = h->new_px; f.img = h->in_img; f.iR_old = h->iR_old; f.good_old = h->good_old;
    f.have_guess = (h->exposure_first > 0 && exposure > 0) ? 1 : 0;
    f.aff_guess = f.have_guess ? logf(exposure / h->exposure_first) : 0.0f;       // :109, the one scalar taken on the host
    f.snapped_threshold = snapped_threshold;
    EDS_HIP_TRY(hipMemsetAsync(h->d_out, 0, sizeof(Result), h->own.st));
    EDS_HIP_TRY(hipEventRecord(h->ev0, h->own.st));
    INI_LAUNCH(h, k_ini_track, f, h->d_carry, h->d_out);
    EDS_HIP_TRY(hipEventRecord(h->ev1, h->own.st));
    EDS_HIP_TRY(hipGetLastError());
    Result back;
    Carry carry;
    EDS_HIP_TRY(hipMemcpyAsync(&back, h->d_out, sizeof(back), hipMemcpyDeviceToHost, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(&carry, h->d_carry, sizeof(carry), hipMemcpyDeviceToHost, h->own.st));
    if (int rc = ini_wait(h)) return rc;
    if (hipEventElapsedTime(&h->kernel_ms, h->ev0, h->ev1) != hipSuccess) { (void)hipGetLastError(); h->kernel_ms = -1.0f; }
    h->carry = carry;
    h->new_set = true;
    back.launches = (int32_t)(h->n_launches - launches0); back.waits = (int32_t)(h->n_waits - waits0);
    std::memcpy(out, &back, sizeof(back));
    return EDS_OK;
}

int eds_ini_get_kernel_ms(const eds_ini* h, float* ms_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!ms_out) return fail(EDS_ERR_INVALID, "null output");
    if (h->kernel_ms < 0.0f) return fail(EDS_ERR_STATE, "eds_ini: no frame was tracked");
    *ms_out = h->kernel_ms;
    return EDS_OK;
}

int eds_ini_get_points(eds_ini* h, int lvl, eds_ini_point* out, int32_t* n_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->points_set[lvl]) return fail(EDS_ERR_STATE, "eds_ini: the level has no points");
    if (int rc = ini_read_back(h, out, h->pts + (size_t)lvl * h->cap, (size_t)h->n[lvl] * sizeof(Pnt))) return rc;
    if (n_out) *n_out = h->n[lvl];
    return EDS_OK;
}

int eds_ini_get_jb(eds_ini* h, int lvl, int which, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (which != 0 && which != 1) return fail(EDS_ERR_INVALID, "which is 0 (JbBuffer) or 1 (JbBuffer_new)");
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->points_set[lvl]) return fail(EDS_ERR_STATE, "eds_ini: the level has no points");
    const int idx = which == 0 ? h->carry.jb_cur[lvl] : 1 - h->carry.jb_cur[lvl];
    return ini_read_back(h, out, h->jb + ((size_t)lvl * 2 + idx) * h->cap * 10, (size_t)h->n[lvl] * 10 * sizeof(float));
}

int eds_ini_get_level(eds_ini* h, int which, int lvl, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (which != 0 && which != 1) return fail(EDS_ERR_INVALID, "which is 0 (the first frame) or 1 (the newest)");
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (which == 0 ? !h->first_set : !h->new_set) return fail(EDS_ERR_STATE, "eds_ini: that frame was never set");
    const Level& L = h->geo.l[lvl];
    const size_t px = (size_t)L.w * L.h;
    std::vector<Px> p(px);
    if (int rc = ini_read_back(h, p.data(), (which == 0 ? h->first_px : h->new_px) + L.off, px * sizeof(Px))) return rc;
    for (size_t i = 0; i < px; ++i) { out[3 * i] = p[i].c; out[3 * i + 1] = p[i].dx; out[3 * i + 2] = p[i].dy; }
    return EDS_OK;
}

}  // extern "C"
