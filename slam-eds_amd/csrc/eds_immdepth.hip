// include/eds_hip_immdepth.h: immature points seeded from a depth map on the device.  The per-pixel loop is eds_immdepth.hpp, shared with
// the host; this file holds the kernels, the state that hangs off an eds_imm and the C entry points.  Built without contraction into
// FMAs (csrc/Makefile).
//
//   k_imd_filter          the selector's list inside the rectangle, in its order: one workgroup sweeps the list 256 at a time with
//                         edsdso::block_rank, as eds_imm_create_points_selected's filter does, and leaves the count on the device.
//   k_imd_nearest         one pixel per lane, edsimd::nearest on the tree in global memory: of edskd::nn's four runtime-indexed stack
//                         arrays 272 bytes a lane live in scratch, the rest in registers (DESIGN §28 has the resource report).
//   k_imd_construct       edsimd::construct per pixel, the alive bytes and the two status counts (integer atomics: no order to fix).
// The three passes read the count the filter left, so nothing waits on the host between them; a count above max_points_per_host makes the
// two later passes return without a store, and the one wait that follows reports it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_immdepth.h"
#include "eds_capi_internal.hpp"
#include "eds_immature_internal.hpp"
#include "eds_immdepth.hpp"
#include "eds_kdbuild_kernel.hpp"
#include "eds_pixsel_internal.hpp"

using edscapi::fail;
using edsimm::Params;
using edsimm::Point;

// one map in tree order
struct ImdTree {
    double *txy = nullptr, *tidp = nullptr;
    int32_t* perm = nullptr;
    size_t cap = 0;
};

struct eds_imd_state {
    bool map_set = false, kd_reserved = false;
    int map_n = 0, tree_on_host = 0;
    ImdTree cur, next;                                 // the map that holds, and the one being built
    double *mxy = nullptr, *midp = nullptr;            // a map given in host memory, uploaded for the device build
    size_t raw_cap = 0;
    int32_t* small = nullptr;                          // [0] the build's n, [1] its flag, [2] the filter's count, [3] GOOD, [4] UNINITIALIZED
    int32_t* nn_index = nullptr;                       // [max_hosts][max_points] what each point took from the map
    float* nn_idepth = nullptr;
    double* nn_distance = nullptr;
    std::vector<int> nn_n;                             // per host: the points of its last eds_imd_create_*, -1 before the first
    int h_n = 0;                                       // the build's n on its way to the device
    int timing = 0;
    int waits = 0, walk_taken = 0;
    float nn_ms = 0.0f, queue_ms = 0.0f;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

namespace {

constexpr int IMD_T = 256;
constexpr int SMALL_WORDS = 8;

__global__ void __launch_bounds__(256) k_imd_filter(const int32_t* __restrict__ uv, const float* __restrict__ type, int n, int x_min, int y_min,
                                                    int x_max, int y_max, int cap, int32_t* __restrict__ out_uv, float* __restrict__ out_type,
                                                    int32_t* __restrict__ n_out) {
    __shared__ int s_wave[256 / 64];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        int u = 0, v = 0;
        bool in = false;
        if (i < n) {
            u = uv[2 * i]; v = uv[2 * i + 1];
            in = u >= x_min && u <= x_max && v >= y_min && v <= y_max;
        }
        int total;
        const int pos = base + edsdso::block_rank<256>(in, s_wave, &total);
        if (in && pos < cap) { out_uv[2 * pos] = u; out_uv[2 * pos + 1] = v; out_type[pos] = type[i]; }
        base += total;
    }
    if (threadIdx.x == 0) *n_out = base;
}

// the pixels of this call: the count on the device (cnt != NULL) or the caller's; -1 when they are more than the handle holds
__device__ __forceinline__ int pixels_of(const int32_t* cnt, int n_host, int cap) {
    const int n = cnt ? *cnt : n_host;
    return n > cap ? -1 : n;
}

__device__ __forceinline__ void store_nearest(const edsimd::Nearest& r, int i, int32_t* __restrict__ index, float* __restrict__ idepth,
                                              double* __restrict__ distance) {
    index[i] = r.index; idepth[i] = r.idepth; distance[i] = r.distance;
}

__global__ void __launch_bounds__(IMD_T) k_imd_nearest(const int32_t* __restrict__ cnt, int n_host, int cap, const int32_t* __restrict__ uv,
                                                              const double* __restrict__ txy, const double* __restrict__ tidp,
                                                              const int32_t* __restrict__ perm, int m, double sx, double sy,
                                                              int32_t* __restrict__ index, float* __restrict__ idepth, double* __restrict__ distance) {
    const int n = pixels_of(cnt, n_host, cap);
    const int i = blockIdx.x * IMD_T + threadIdx.x;
    if (i >= n) return;
    store_nearest(edsimd::nearest(txy, tidp, perm, m, uv[2 * i], uv[2 * i + 1], sx, sy), i, index, idepth, distance);
}

__global__ void __launch_bounds__(IMD_T) k_imd_construct(const int32_t* __restrict__ cnt, int n_host, int cap, Point* __restrict__ pts,
                                                         const float* __restrict__ c, int W, int H, Params s, const int32_t* __restrict__ uv,
                                                         const float* __restrict__ type, int has_map, int32_t* __restrict__ index,
                                                         float* __restrict__ idepth, double* __restrict__ distance, uint8_t* __restrict__ alive,
                                                         int32_t* __restrict__ status_counts) {
    __shared__ int s_cnt[2];
    const int n = pixels_of(cnt, n_host, cap);
    if ((int)(blockIdx.x * IMD_T) >= n) return;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * IMD_T + threadIdx.x;
    if (i < n) {
        edsimd::Nearest nn = edsimd::none();
        if (has_map) { nn.pos = 0; nn.index = index[i]; nn.idepth = idepth[i]; nn.distance = distance[i]; }
        else store_nearest(nn, i, index, idepth, distance);
        Point p;
        edsimd::construct(p, c, W, H, s, uv[2 * i], uv[2 * i + 1], type[i], nn);
        pts[i] = p;
        alive[i] = (uint8_t)p.alive;
        if (p.alive && p.status == edsimm::GOOD) atomicAdd(&s_cnt[0], 1);
        if (p.alive && p.status == edsimm::UNINITIALIZED) atomicAdd(&s_cnt[1], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&status_counts[threadIdx.x], s_cnt[threadIdx.x]);
}

int check_host(const eds_imm* h, int host) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (host < 0 || host >= h->max_hosts) return fail(EDS_ERR_INVALID, "host " + std::to_string(host) + " outside 0 .. " + std::to_string(h->max_hosts - 1));
    return EDS_OK;
}

// the state, allocated by the first call that needs it
int state_of(eds_imm* h, eds_imd_state** out) {
    if (h->imd) { *out = h->imd; return EDS_OK; }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    eds_imd_state* s = new eds_imd_state;
    const size_t np = (size_t)h->max_hosts * h->max_points;
    if (!h->own.alloc({{(void**)&s->small, SMALL_WORDS * sizeof(int32_t)},
                       {(void**)&s->nn_index, np * sizeof(int32_t)},
                       {(void**)&s->nn_idepth, np * sizeof(float)},
                       {(void**)&s->nn_distance, np * sizeof(double)}})) {
        delete s;
        return fail(EDS_ERR_HIP, "eds_imd: the device refused an allocation");
    }
    s->nn_n.assign(h->max_hosts, -1);
    h->imd = s;
    *out = s;
    return EDS_OK;
}

int wait(eds_imm* h, eds_imd_state* s) {
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    ++s->waits;
    return EDS_OK;
}

int ensure_tree(eds_imm* h, ImdTree& t, size_t n) {
    if (t.cap >= n) return EDS_OK;
    h->own.release(t.txy); h->own.release(t.tidp); h->own.release(t.perm);
    t.cap = 0;
    if (!h->own.alloc({{(void**)&t.txy, n * 16}, {(void**)&t.tidp, n * 8}, {(void**)&t.perm, n * 4}}))
        return fail(EDS_ERR_HIP, "eds_imd_set_depth_map: the device refused an allocation");
    t.cap = n;
    return EDS_OK;
}

int ensure_raw(eds_imm* h, eds_imd_state* s, size_t n) {
    if (s->raw_cap >= n) return EDS_OK;
    h->own.release(s->mxy); h->own.release(s->midp);
    s->raw_cap = 0;
    if (!h->own.alloc({{(void**)&s->mxy, n * 16}, {(void**)&s->midp, n * 8}}))
        return fail(EDS_ERR_HIP, "eds_imd_set_depth_map: the device refused an allocation");
    s->raw_cap = n;
    return EDS_OK;
}

void take_next(eds_imd_state* s, int n, int on_host) {
    const ImdTree t = s->cur;
    s->cur = s->next; s->next = t;
    s->map_set = true; s->map_n = n; s->tree_on_host = on_host;
}

int ensure_events(eds_imd_state* s) {
    for (hipEvent_t& e : s->ev) if (!e) EDS_HIP_TRY(hipEventCreate(&e));
    return EDS_OK;
}

// Everything a create call does once its pixel list is known to be in (or on its way into) the staging buffers: n_list < 0 means the
// selector's list, filtered here.
int create(eds_imm* h, int host, const eds_sel* sel, int x_min, int y_min, int x_max, int y_max, int n_list, const int32_t* uv, const float* type,
           int on_device, const double* scale, uint8_t* alive_out, int* n_out, int32_t* status_counts_out) {
    eds_imd_state* s = h->imd;
    if (!s || !s->map_set) return fail(EDS_ERR_STATE, "no depth map: eds_imd_set_depth_map first");
    if (!h->host_set[host]) return fail(EDS_ERR_STATE, "host " + std::to_string(host) + " has no image");
    double sx = 1.0, sy = 1.0;
    if (scale) { sx = scale[0]; sy = scale[1]; }
    if (!std::isfinite(sx) || !std::isfinite(sy)) return fail(EDS_ERR_INVALID, "the scale is not finite");
    const int m = s->map_n;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    s->waits = 0; s->walk_taken = 0; s->nn_ms = s->queue_ms = 0.0f;
    const int ub = sel ? (sel->n_sel < h->max_points ? sel->n_sel : h->max_points) : n_list;      // the pixels this call can create
    int32_t res[3] = {0, 0, 0};
    std::vector<uint8_t> alive((size_t)ub);
    if (ub > 0) {
        hipStream_t st = h->own.st;
        const bool timed = s->timing != 0;
        if (timed) { if (int rc = ensure_events(s)) return rc; }
        if (timed) EDS_HIP_TRY(hipEventRecord(s->ev[0], st));
        EDS_HIP_TRY(hipMemsetAsync(s->small + 2, 0, 3 * sizeof(int32_t), st));
        const int32_t* cnt = nullptr;
        if (sel) {
            // the staging buffers hold nothing a caller can see; the selector's calls have returned, so its list is complete
            hipLaunchKernelGGL(k_imd_filter, dim3(1), dim3(256), 0, st, sel->uv, sel->type, sel->n_sel, x_min, y_min, x_max, y_max, h->max_points, h->in_uv,
                               h->in_type, s->small + 2);
            cnt = s->small + 2;
        } else {
            const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
            EDS_HIP_TRY(hipMemcpyAsync(h->in_uv, uv, (size_t)n_list * 2 * sizeof(int32_t), kind, st));
            EDS_HIP_TRY(hipMemcpyAsync(h->in_type, type, (size_t)n_list * sizeof(float), kind, st));
        }
        const size_t po = (size_t)host * h->max_points;
        const unsigned nb = edscapi::blocks(ub, IMD_T);
        if (timed) EDS_HIP_TRY(hipEventRecord(s->ev[1], st));
        if (m > 0) {
            hipLaunchKernelGGL(k_imd_nearest, dim3(nb), dim3(IMD_T), 0, st, cnt, n_list, h->max_points, h->in_uv, s->cur.txy, s->cur.tidp, s->cur.perm, m,
                               sx, sy, s->nn_index + po, s->nn_idepth + po, s->nn_distance + po);
            s->walk_taken = EDS_IMD_WALK_GLOBAL;
        }
        if (timed) EDS_HIP_TRY(hipEventRecord(s->ev[2], st));
        hipLaunchKernelGGL(k_imd_construct, dim3(nb), dim3(IMD_T), 0, st, cnt, n_list, h->max_points, h->points + po,
                           h->host_c + (size_t)h->W * h->H * host, h->W, h->H, h->prm, h->in_uv, h->in_type, m > 0 ? 1 : 0, s->nn_index + po, s->nn_idepth + po,
                           s->nn_distance + po, h->in_alive, s->small + 3);
        EDS_HIP_TRY(hipGetLastError());
        EDS_HIP_TRY(hipMemcpyAsync(res, s->small + 2, sizeof(res), hipMemcpyDeviceToHost, st));
        EDS_HIP_TRY(hipMemcpyAsync(alive.data(), h->in_alive, (size_t)ub, hipMemcpyDeviceToHost, st));
        if (timed) EDS_HIP_TRY(hipEventRecord(s->ev[3], st));
        if (int rc = wait(h, s)) return rc;
        if (timed) {
            EDS_HIP_TRY(hipEventElapsedTime(&s->nn_ms, s->ev[1], s->ev[2]));
            EDS_HIP_TRY(hipEventElapsedTime(&s->queue_ms, s->ev[0], s->ev[3]));
        }
    }
    const int n = sel ? (ub > 0 ? res[0] : 0) : n_list;
    if (n > h->max_points)
        return fail(EDS_ERR_INVALID, std::to_string(n) + " selected points, the handle holds 0 .. " + std::to_string(h->max_points) + " per host");
    edsimm_internal::act_invalidate(h);
    h->n[host] = n;
    s->nn_n[host] = n;
    if (n_out) *n_out = n;
    if (alive_out && n > 0) std::memcpy(alive_out, alive.data(), (size_t)n);
    if (status_counts_out) { status_counts_out[0] = res[1]; status_counts_out[1] = res[2]; }
    return EDS_OK;
}

}  // namespace

namespace edsimm_internal {
// the state's device memory belongs to the eds_imm's owner, which has freed it; the events and the struct are ours
void imd_release(eds_imm* h) {
    if (!h->imd) return;
    for (hipEvent_t e : h->imd->ev) if (e) (void)hipEventDestroy(e);
    delete h->imd;
    h->imd = nullptr;
}
}  // namespace edsimm_internal

extern "C" {

int eds_imd_abi_version(void) { return EDS_HIP_IMMDEPTH_ABI_VERSION; }

int eds_imd_set_depth_map(eds_imm* h, int n, const double* depth_xy, const double* depth_idp, int on_device, int* tree_on_host) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (n < 0) return fail(EDS_ERR_INVALID, "negative depth-map size");
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    if (n > 0 && (!depth_xy || !depth_idp)) return fail(EDS_ERR_INVALID, "null depth map");
    if (n > 0 && ((reinterpret_cast<uintptr_t>(depth_xy) | reinterpret_cast<uintptr_t>(depth_idp)) & 7))
        return fail(EDS_ERR_INVALID, "a depth-map array is not aligned to a double");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (n > 0 && on_device) {
        if (int rc = eds_dev_check_range(h->own.dev, depth_xy, (size_t)n * 16)) return rc;
        if (int rc = eds_dev_check_range(h->own.dev, depth_idp, (size_t)n * 8)) return rc;
    }
    if (n > 0 && !on_device && !edsimd::map_finite(depth_xy, n)) return fail(EDS_ERR_INVALID, "a depth-map coordinate is not finite");
    eds_imd_state* s = nullptr;
    if (int rc = state_of(h, &s)) return rc;
    if (n == 0) {
        s->map_set = true; s->map_n = 0; s->tree_on_host = 0;
        if (tree_on_host) *tree_on_host = 0;
        return EDS_OK;
    }
    if (int rc = ensure_tree(h, s->next, (size_t)n)) return rc;
    hipStream_t st = h->own.st;
    bool on_host = n > edskdb::CAPACITY;
    if (!on_host) {
        const double *dxy = depth_xy, *didp = depth_idp;
        if (!on_device) {
            if (int rc = ensure_raw(h, s, (size_t)n)) return rc;
            EDS_HIP_TRY(hipMemcpyAsync(s->mxy, depth_xy, (size_t)n * 16, hipMemcpyHostToDevice, st));
            EDS_HIP_TRY(hipMemcpyAsync(s->midp, depth_idp, (size_t)n * 8, hipMemcpyHostToDevice, st));
            dxy = s->mxy; didp = s->midp;
        }
        if (!s->kd_reserved) {
            if (int rc = kd_build_reserve()) return rc;
            s->kd_reserved = true;
        }
        s->h_n = n;
        int flag = 0;
        EDS_HIP_TRY(hipMemcpyAsync(s->small, &s->h_n, sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (int rc = kd_build_launch(st, 1, dxy, didp, (size_t)n, s->small, n, (size_t)n, s->next.perm, s->next.txy, s->next.tidp, s->small + 1)) return rc;
        EDS_HIP_TRY(hipMemcpyAsync(&flag, s->small + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        EDS_HIP_TRY(hipStreamSynchronize(st));
        on_host = flag != 0;
    }
    if (on_host) {
        // ambiguous, not finite or beyond the capacity: the map taken back and built by std::nth_element, as eds_kfs_build_tree does
        std::vector<double> dl_xy, dl_idp;
        const double *xy = depth_xy, *idp = depth_idp;
        if (on_device) {
            dl_xy.resize(2 * (size_t)n); dl_idp.resize((size_t)n);
            EDS_HIP_TRY(hipMemcpyAsync(dl_xy.data(), depth_xy, (size_t)n * 16, hipMemcpyDeviceToHost, st));
            EDS_HIP_TRY(hipMemcpyAsync(dl_idp.data(), depth_idp, (size_t)n * 8, hipMemcpyDeviceToHost, st));
            EDS_HIP_TRY(hipStreamSynchronize(st));
            xy = dl_xy.data(); idp = dl_idp.data();
            if (!edsimd::map_finite(xy, n)) return fail(EDS_ERR_INVALID, "a depth-map coordinate is not finite");
        }
        std::vector<int> perm((size_t)n);
        edskd::build_tree(xy, n, perm.data());
        std::vector<double> txy(2 * (size_t)n), tidp((size_t)n);
        for (int p = 0; p < n; ++p) {
            const size_t i = (size_t)perm[p];
            txy[2 * (size_t)p] = xy[2 * i]; txy[2 * (size_t)p + 1] = xy[2 * i + 1]; tidp[p] = idp[i];
        }
        EDS_HIP_TRY(hipMemcpyAsync(s->next.perm, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        EDS_HIP_TRY(hipMemcpyAsync(s->next.txy, txy.data(), (size_t)n * 16, hipMemcpyHostToDevice, st));
        EDS_HIP_TRY(hipMemcpyAsync(s->next.tidp, tidp.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        EDS_HIP_TRY(hipStreamSynchronize(st));
    }
    take_next(s, n, on_host ? 1 : 0);
    if (tree_on_host) *tree_on_host = on_host ? 1 : 0;
    return EDS_OK;
}

int eds_imd_create_points_selected(eds_imm* h, int host, const eds_sel* sel, int x_min, int y_min, int x_max, int y_max, const double* scale,
                                   uint8_t* alive_out, int* n_out, int32_t* status_counts_out) {
    if (int rc = check_host(h, host)) return rc;
    if (!sel) return fail(EDS_ERR_INVALID, "null eds_sel handle");
    if (sel->H != h->H || sel->W != h->W || sel->own.dev != h->own.dev) return fail(EDS_ERR_INVALID, "the selector and the points differ in H, W or device");
    if (x_min < 0 || y_min < 0 || x_max >= h->W || y_max >= h->H || x_min > x_max || y_min > y_max)
        return fail(EDS_ERR_INVALID, "the rectangle lies inside the image, min <= max");
    if (!sel->sel_valid) return fail(EDS_ERR_STATE, "no selection: eds_sel_make_maps first");
    if (!sel->hist_valid) return fail(EDS_ERR_STATE, "the selection is stale: the selector's image or parameters changed since eds_sel_make_maps");
    return create(h, host, sel, x_min, y_min, x_max, y_max, -1, nullptr, nullptr, 0, scale, alive_out, n_out, status_counts_out);
}

int eds_imd_create_points(eds_imm* h, int host, int n, const int32_t* uv, const float* type, int on_device, const double* scale, uint8_t* alive_out,
                          int32_t* status_counts_out) {
    if (int rc = check_host(h, host)) return rc;
    if (n < 0 || n > h->max_points)
        return fail(EDS_ERR_INVALID, std::to_string(n) + " points, the handle holds 0 .. " + std::to_string(h->max_points) + " per host");
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    if (n > 0 && (!uv || !type)) return fail(EDS_ERR_INVALID, "uv and type are required");
    if (n > 0 && on_device) {
        if ((reinterpret_cast<uintptr_t>(uv) | reinterpret_cast<uintptr_t>(type)) & 3) return fail(EDS_ERR_INVALID, "uv or type is not aligned to 4 bytes");
        EDS_HIP_TRY(hipSetDevice(h->own.dev));
        if (int rc = eds_dev_check_range(h->own.dev, uv, (size_t)n * 8)) return rc;
        if (int rc = eds_dev_check_range(h->own.dev, type, (size_t)n * 4)) return rc;
    }
    return create(h, host, nullptr, 0, 0, 0, 0, n, uv, type, on_device, scale, alive_out, nullptr, status_counts_out);
}

int eds_imd_get_nearest(eds_imm* h, int host, int32_t* index_out, float* idepth_out, double* distance_out) {
    if (int rc = check_host(h, host)) return rc;
    eds_imd_state* s = h->imd;
    if (!s || s->nn_n[host] < 0) return fail(EDS_ERR_STATE, "host " + std::to_string(host) + " holds no points of an eds_imd_create_* call");
    if (s->nn_n[host] != h->n[host]) return fail(EDS_ERR_STATE, "the points of host " + std::to_string(host) + " were replaced since eds_imd_create_*");
    const size_t n = (size_t)s->nn_n[host], po = (size_t)host * h->max_points;
    if (int rc = edscapi::read_back(h->own, index_out, s->nn_index + po, n * sizeof(int32_t))) return rc;
    if (int rc = edscapi::read_back(h->own, idepth_out, s->nn_idepth + po, n * sizeof(float))) return rc;
    return edscapi::read_back(h->own, distance_out, s->nn_distance + po, n * sizeof(double));
}

int eds_imd_get_tree(eds_imm* h, int32_t* perm_out, double* txy_out, double* tidp_out) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    eds_imd_state* s = h->imd;
    if (!s || !s->map_set) return fail(EDS_ERR_STATE, "no depth map: eds_imd_set_depth_map first");
    const size_t n = (size_t)s->map_n;
    if (int rc = edscapi::read_back(h->own, perm_out, s->cur.perm, n * sizeof(int32_t))) return rc;
    if (int rc = edscapi::read_back(h->own, txy_out, s->cur.txy, n * 16)) return rc;
    return edscapi::read_back(h->own, tidp_out, s->cur.tidp, n * 8);
}

int eds_imd_set_debug(eds_imm* h, int timing) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (timing != 0 && timing != 1) return fail(EDS_ERR_INVALID, "timing is 0 or 1");
    eds_imd_state* s = nullptr;
    if (int rc = state_of(h, &s)) return rc;
    s->timing = timing;
    return EDS_OK;
}

int eds_imd_get_info(eds_imm* h, eds_imd_info* info) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!info) return fail(EDS_ERR_INVALID, "null output");
    std::memset(info, 0, sizeof(*info));
    const eds_imd_state* s = h->imd;
    if (!s) return EDS_OK;
    info->map_set = s->map_set ? 1 : 0; info->map_n = s->map_n; info->tree_on_host = s->tree_on_host;
    info->waits = s->waits; info->walk = s->walk_taken;
    info->nn_kernel_ms = s->nn_ms; info->queue_ms = s->queue_ms;
    return EDS_OK;
}

}  // extern "C"
