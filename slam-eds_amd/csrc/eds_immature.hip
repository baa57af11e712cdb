// include/eds_hip_immature.h: DSO's immature points on the device.  The per-point arithmetic is eds_immature.hpp, shared with the host;
// this file holds the kernels and the C entry points.  Built without contraction into FMAs (csrc/Makefile).
//
// k_imm_trace maps ONE WAVEFRONT to one point.  What traceOn decides before the search (OOB, SKIPPED, BADCONDITION, the scale test) is
// computed by every lane from wave-uniform values, so a point that exits early retires its whole wavefront before any image load.  In
// the discrete search lane i owns step i (a second pass owns steps 64 .. 98): it reaches its position by i sequential additions of
// (dx, dy), as the serial loop does, and sums its 8 taps in pattern order, so every energy has the serial sum's rounding.  The arg-min is a
// butterfly on (energy, index) that prefers the lower index on a tie — the first index of the minimum, the serial loop's strict < —
// and the second-best score a butterfly minimum over the lanes outside the radius.  The Gauss-Newton steps are serial by nature: every
// lane runs them on the same values (the loads are wave-uniform, one request each), which keeps one code path with the host and costs
// nothing a single active lane would save.  errors[100] of the reference is one or two registers per lane.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_immature.h"
#include "eds_capi_internal.hpp"
#include "eds_immature.hpp"
#include "eds_immature_internal.hpp"
#include "eds_pixsel_internal.hpp"

using edscapi::fail;
using edscapi::read_back;
using edsimm::Frame;
using edsimm::Grad;
using edsimm::Line;
using edsimm::Params;
using edsimm::Point;
using edsimm::Pre;

static_assert(sizeof(Point) == 128, "one point is 32 words");
static_assert(sizeof(Params) == sizeof(eds_imm_params), "edsimm::Params is eds_imm_params member for member");
static_assert(sizeof(Pre) == 64, "one host's precalc is 16 words");

namespace {

constexpr int WAVE = 64;
constexpr int TRACE_THREADS = 256;                     // four points per workgroup

__global__ void __launch_bounds__(256) k_imm_gradient(const float* __restrict__ c, Grad* __restrict__ g, int W, int H, int frames) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t px = (int64_t)W * H;
    if (t >= px * frames) return;
    const int64_t f = t / px;
    const int i = (int)(t - f * px);
    g[t] = edsimm::gradient_at(c + f * px, W, H, i);
}

__global__ void __launch_bounds__(256) k_imm_construct(Point* __restrict__ pts, const float* __restrict__ c, int W, int H, Params s, int n,
                                                       const int32_t* __restrict__ uv, const float* __restrict__ type,
                                                       const float* __restrict__ idepth, const double* __restrict__ distance, int has_depth,
                                                       uint8_t* __restrict__ alive) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Point p;
    edsimm::construct(p, c, W, H, s, uv[2 * i], uv[2 * i + 1], type[i], has_depth != 0, has_depth ? idepth[i] : 0.0f,
                      has_depth ? distance[i] : 0.0);
    pts[i] = p;
    alive[i] = (uint8_t)p.alive;
}

// eds_imm_create_points_selected: the entries of a selection list (row-major order) inside the inclusive rectangle, in their order, as
// eds_imm_create_points' staged inputs.  One workgroup walks the list 256 at a time, so the order is the list's; an entry past `cap`
// is counted and not stored.
__global__ void __launch_bounds__(256) k_imm_filter_rect(const int32_t* __restrict__ uv, const float* __restrict__ type, int n, int x_min, int y_min,
                                                         int x_max, int y_max, int cap, int32_t* __restrict__ out_uv, float* __restrict__ out_type,
                                                         int32_t* __restrict__ n_out) {
    __shared__ int s_wave[256 / WAVE];
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

__global__ void __launch_bounds__(TRACE_THREADS) k_imm_trace(Point* __restrict__ points, int max_points, int first_host,
                                                             const Pre* __restrict__ pre, const float* __restrict__ target_c,
                                                             const Grad* __restrict__ target_g, int W, int H, Params s) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int pi = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TRACE_THREADS / WAVE) + (threadIdx.x / WAVE)));
    const Pre m = pre[blockIdx.y];
    if (pi >= m.n) return;
    Point* gp = points + ((size_t)(first_host + blockIdx.y) * max_points + pi);
    Point p = *gp;
    if (!p.alive) return;
    Line L;
    if (!edsimm::trace_prologue(p, s, W, H, m, L)) {
        if (lane == 0) *gp = p;
        return;
    }
    const size_t px = (size_t)W * H;
    Frame f;
    f.c = target_c + px * m.target;
    f.g = target_g + px * m.target;

    // the discrete search: lane i at step i, then at step 64 + i
    float ptx = L.ptx, pty = L.pty;
    for (int k = 0; k < lane; ++k) { ptx += L.dx; pty += L.dy; }
    const float px0 = ptx, py0 = pty;
    const float e0 = lane < L.numSteps ? edsimm::step_energy(p, s, f.c, W, H, m, L, ptx, pty) : 0.0f;
    float px1 = 0.0f, py1 = 0.0f, e1 = 0.0f;
    if (L.numSteps > WAVE) {
        for (int k = 0; k < WAVE; ++k) { ptx += L.dx; pty += L.dy; }
        px1 = ptx; py1 = pty;
        if (lane + WAVE < L.numSteps) e1 = edsimm::step_energy(p, s, f.c, W, H, m, L, ptx, pty);
    }
    const bool in0 = lane < L.numSteps, in1 = lane + WAVE < L.numSteps;

    // the first index of the minimum among the energies `energy < bestEnergy` can accept
    constexpr int NONE = 1 << 20;
    float ke = INFINITY;
    int ki = NONE;
    if (in0 && edsimm::can_be_best(e0)) { ke = e0; ki = lane; }
    if (in1 && edsimm::can_be_best(e1) && e1 < ke) { ke = e1; ki = lane + WAVE; }
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const float oe = __shfl_xor(ke, d);
        const int oi = __shfl_xor(ki, d);
        if (oe < ke || (oe == ke && oi < ki)) { ke = oe; ki = oi; }
    }
    int bestIdx = -1;
    float bestU = 0, bestV = 0, bestEnergy = 1e10f;
    const int src = ki & (WAVE - 1);
    const float u0 = __shfl(px0, src), v0 = __shfl(py0, src), u1 = __shfl(px1, src), v1 = __shfl(py1, src);
    if (ki != NONE) {
        bestIdx = ki;
        bestEnergy = ke;
        bestU = ki < WAVE ? u0 : u1;
        bestV = ki < WAVE ? v0 : v1;
    }
    float secondBest = 1e10f;
    if (in0 && edsimm::outside_radius(lane, bestIdx, s.min_trace_test_radius) && e0 < secondBest) secondBest = e0;
    if (in1 && edsimm::outside_radius(lane + WAVE, bestIdx, s.min_trace_test_radius) && e1 < secondBest) secondBest = e1;
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const float o = __shfl_xor(secondBest, d);
        if (o < secondBest) secondBest = o;
    }

    edsimm::trace_epilogue(p, s, f, W, H, m, L, bestU, bestV, bestEnergy, secondBest);
    if (lane == 0) *gp = p;
}

// per host the number of live points that hold each status (integer atomics in LDS: the counts do not depend on their order)
__global__ void __launch_bounds__(256) k_imm_summary(const Point* __restrict__ points, int max_points, int first_host,
                                                     const Pre* __restrict__ pre, int32_t* __restrict__ out) {
    __shared__ int cnt[edsimm::NUM_STATUS];
    if (threadIdx.x < edsimm::NUM_STATUS) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int n = pre[blockIdx.x].n;
    const Point* pts = points + (size_t)(first_host + blockIdx.x) * max_points;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int st = pts[i].status;
        if (pts[i].alive && st >= 0 && st < edsimm::NUM_STATUS) atomicAdd(&cnt[st], 1);
    }
    __syncthreads();
    if (threadIdx.x < edsimm::NUM_STATUS) out[blockIdx.x * edsimm::NUM_STATUS + threadIdx.x] = cnt[threadIdx.x];
}

int check_host(const eds_imm* h, int host) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (host < 0 || host >= h->max_hosts) return fail(EDS_ERR_INVALID, "host " + std::to_string(host) + " outside 0 .. " + std::to_string(h->max_hosts - 1));
    return EDS_OK;
}

int set_images(eds_imm* h, bool target, int first, int count, const float* images, int64_t fs, int64_t rs, int on_device) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    const int cap = target ? h->max_targets : h->max_hosts;
    if (first < 0 || count < 1 || first > cap - count)
        return fail(EDS_ERR_INVALID, "frames " + std::to_string(first) + " .. +" + std::to_string(count) + " outside 0 .. " + std::to_string(cap - 1));
    const int H = h->H, W = h->W;
    if (int rc = edscapi::check_images(h->own.dev, H, W, count, images, &rs, &fs, on_device, "images", "bad image strides")) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t px = (size_t)W * H;
    float* c = (target ? h->target_c : h->host_c) + px * first;
    Grad* g = (target ? h->target_g : h->host_g) + px * first;
    for (int b = 0; b < count; ++b)
        if (int rc = edscapi::upload_image(h->own, c + px * b, H, W, images + (int64_t)b * fs, rs, on_device)) return rc;
    const int64_t total = (int64_t)px * count;
    hipLaunchKernelGGL(k_imm_gradient, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->own.st, c, g, W, H, count);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    std::vector<uint8_t>& set = target ? h->target_set : h->host_set;
    for (int b = 0; b < count; ++b) set[first + b] = 1;
    if (!target) edsimm_internal::act_invalidate(h);
    return EDS_OK;
}

// the points of `host` on the host; waits
int read_points(eds_imm* h, int host, std::vector<Point>& out) {
    out.resize((size_t)h->n[host]);
    return read_back(h->own, out.data(), h->points + (size_t)host * h->max_points, out.size() * sizeof(Point));
}

// the constructor kernel over the n staged inputs (in_uv, in_type, and in_idepth, in_distance for the second constructor)
int construct_staged(eds_imm* h, int host, int n, bool has_depth, uint8_t* alive_out) {
    h->n[host] = 0;                                     // what the host held is gone once the kernel is queued
    hipLaunchKernelGGL(k_imm_construct, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->own.st, h->points + (size_t)host * h->max_points,
                       h->host_c + (size_t)h->W * h->H * host, h->W, h->H, h->prm, n, h->in_uv, h->in_type, h->in_idepth, h->in_distance,
                       has_depth ? 1 : 0, h->in_alive);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<uint8_t> alive((size_t)n);
    if (int rc = read_back(h->own, alive.data(), h->in_alive, (size_t)n)) return rc;
    if (alive_out) std::memcpy(alive_out, alive.data(), (size_t)n);
    h->n[host] = n;
    return EDS_OK;
}

bool all_finite(const float* x, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false;
    return true;
}

}  // namespace

extern "C" {

int eds_imm_abi_version(void) { return EDS_HIP_IMMATURE_ABI_VERSION; }

void eds_imm_params_default(eds_imm_params* p) {
    if (!p) return;
    const Params d = edsimm::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_imm_create(int device, int H, int W, int max_hosts, int max_points_per_host, int max_targets, eds_imm** imm) {
    if (!imm) return fail(EDS_ERR_INVALID, "null output");
    *imm = nullptr;
    if (H < 8 || W < 8 || H > 16384 || W > 16384) return fail(EDS_ERR_INVALID, "H and W are 8 .. 16384");
    if (max_hosts < 1 || max_points_per_host < 1 || max_targets < 1 || max_hosts > 4096 || max_targets > 4096 || max_points_per_host > (1 << 22))
        return fail(EDS_ERR_INVALID, "max_hosts and max_targets are 1 .. 4096, max_points_per_host 1 .. 4194304");
    eds_imm* h = new eds_imm;
    if (int rc = h->own.open(device)) { delete h; return rc; }
    h->H = H; h->W = W; h->max_hosts = max_hosts; h->max_points = max_points_per_host; h->max_targets = max_targets;
    h->prm = edsimm::params_default();
    h->n.assign(max_hosts, 0);
    h->host_set.assign(max_hosts, 0);
    h->target_set.assign(max_targets, 0);
    const size_t px = (size_t)H * W, mp = (size_t)max_points_per_host;
    const bool ok = h->own.alloc({{(void**)&h->host_c, px * max_hosts * sizeof(float)},
                                  {(void**)&h->host_g, px * max_hosts * sizeof(Grad)},
                                  {(void**)&h->target_c, px * max_targets * sizeof(float)},
                                  {(void**)&h->target_g, px * max_targets * sizeof(Grad)},
                                  {(void**)&h->points, mp * max_hosts * sizeof(Point)},
                                  {(void**)&h->pre, (size_t)max_hosts * sizeof(Pre)},
                                  {(void**)&h->summary, (size_t)max_hosts * edsimm::NUM_STATUS * sizeof(int32_t)},
                                  {(void**)&h->in_distance, mp * sizeof(double)},
                                  {(void**)&h->in_uv, mp * 2 * sizeof(int32_t)},
                                  {(void**)&h->in_type, mp * sizeof(float)},
                                  {(void**)&h->in_idepth, mp * sizeof(float)},
                                  {(void**)&h->in_alive, mp}});
    if (!ok) {
        eds_imm_destroy(h);
        return fail(EDS_ERR_HIP, "eds_imm_create: the device refused a stream or an allocation");
    }
    *imm = h;
    return EDS_OK;
}

void eds_imm_destroy(eds_imm* h) {
    if (!h) return;
    h->own.close();
    edsimm_internal::act_release(h);
    edsmap_internal::release(h->map);
    edsimm_internal::imd_release(h);
    delete h;
}

int eds_imm_set_params(eds_imm* h, const eds_imm_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null parameters");
    Params s;
    std::memcpy(&s, p, sizeof(s));
    if (!edsimm::params_valid(s))
        return fail(EDS_ERR_INVALID, "parameters: every float finite; stepsize, max_pix_search, huber_th, outlier_th_sum_component > 0; "
                                     "gn_iterations 0 .. 16; min_trace_test_radius 0 .. 99");
    h->prm = s;
    return EDS_OK;
}

int eds_imm_get_params(const eds_imm* h, eds_imm_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(p, &h->prm, sizeof(*p));
    return EDS_OK;
}

int eds_imm_set_host_images(eds_imm* h, int first, int count, const float* images, int64_t frame_stride, int64_t row_stride, int on_device) {
    return set_images(h, false, first, count, images, frame_stride, row_stride, on_device);
}

int eds_imm_set_target_images(eds_imm* h, int first, int count, const float* images, int64_t frame_stride, int64_t row_stride, int on_device) {
    return set_images(h, true, first, count, images, frame_stride, row_stride, on_device);
}

int eds_imm_create_points(eds_imm* h, int host, int n, const int32_t* uv, const float* type, const float* idepth, const double* distance,
                          uint8_t* alive_out) {
    if (int rc = check_host(h, host)) return rc;
    if (n < 0 || n > h->max_points)
        return fail(EDS_ERR_INVALID, std::to_string(n) + " points, the handle holds 0 .. " + std::to_string(h->max_points) + " per host");
    if (n > 0 && (!uv || !type)) return fail(EDS_ERR_INVALID, "uv and type are required");
    if ((idepth == nullptr) != (distance == nullptr)) return fail(EDS_ERR_INVALID, "idepth and distance come together");
    if (!h->host_set[host]) return fail(EDS_ERR_STATE, "host " + std::to_string(host) + " has no image");
    edsimm_internal::act_invalidate(h);
    if (n == 0) { h->n[host] = 0; return EDS_OK; }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->in_uv, uv, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->in_type, type, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    if (idepth) {
        EDS_HIP_TRY(hipMemcpyAsync(h->in_idepth, idepth, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->in_distance, distance, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    }
    return construct_staged(h, host, n, idepth != nullptr, alive_out);
}

int eds_imm_create_points_selected(eds_imm* h, int host, const eds_sel* sel, int x_min, int y_min, int x_max, int y_max, uint8_t* alive_out,
                                   int* n_out) {
    if (int rc = check_host(h, host)) return rc;
    if (!sel) return fail(EDS_ERR_INVALID, "null eds_sel handle");
    if (sel->H != h->H || sel->W != h->W || sel->own.dev != h->own.dev) return fail(EDS_ERR_INVALID, "the selector and the points differ in H, W or device");
    if (x_min < 0 || y_min < 0 || x_max >= h->W || y_max >= h->H || x_min > x_max || y_min > y_max)
        return fail(EDS_ERR_INVALID, "the rectangle lies inside the image, min <= max");
    if (!sel->sel_valid) return fail(EDS_ERR_STATE, "no selection: eds_sel_make_maps first");
    if (!h->host_set[host]) return fail(EDS_ERR_STATE, "host " + std::to_string(host) + " has no image");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    int32_t n = 0;
    if (sel->n_sel > 0) {
        // the staging buffers hold nothing a caller can see; the selector's calls have returned, so its list is complete
        hipLaunchKernelGGL(k_imm_filter_rect, dim3(1), dim3(256), 0, h->own.st, sel->uv, sel->type, sel->n_sel, x_min, y_min, x_max, y_max, h->max_points,
                           h->in_uv, h->in_type, h->summary);
        EDS_HIP_TRY(hipGetLastError());
        if (int rc = read_back(h->own, &n, h->summary, sizeof(n))) return rc;
    }
    if (n > h->max_points)
        return fail(EDS_ERR_INVALID, std::to_string(n) + " selected points, the handle holds 0 .. " + std::to_string(h->max_points) + " per host");
    edsimm_internal::act_invalidate(h);
    if (n_out) *n_out = n;
    if (n == 0) { h->n[host] = 0; return EDS_OK; }
    return construct_staged(h, host, n, false, alive_out);
}

int eds_imm_num_points(const eds_imm* h, int host, int* n) {
    if (int rc = check_host(h, host)) return rc;
    if (!n) return fail(EDS_ERR_INVALID, "null output");
    *n = h->n[host];
    return EDS_OK;
}

int eds_imm_trace(eds_imm* h, int first_host, int count, const int32_t* target_index, const float* KRKi, const float* Kt, const float* aff,
                  int32_t* summary_out) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (first_host < 0 || count < 1 || first_host > h->max_hosts - count)
        return fail(EDS_ERR_INVALID, "hosts " + std::to_string(first_host) + " .. +" + std::to_string(count) + " outside 0 .. " + std::to_string(h->max_hosts - 1));
    if (!target_index || !KRKi || !Kt || !aff) return fail(EDS_ERR_INVALID, "target_index, KRKi, Kt and aff are required");
    for (int b = 0; b < count; ++b)
        if (target_index[b] < 0 || target_index[b] >= h->max_targets)
            return fail(EDS_ERR_INVALID, "target " + std::to_string(target_index[b]) + " outside 0 .. " + std::to_string(h->max_targets - 1));
    if (!all_finite(KRKi, 9 * count) || !all_finite(Kt, 3 * count) || !all_finite(aff, 2 * count))
        return fail(EDS_ERR_INVALID, "KRKi, Kt or aff is not finite");
    for (int b = 0; b < count; ++b)
        if (!h->target_set[target_index[b]]) return fail(EDS_ERR_STATE, "target " + std::to_string(target_index[b]) + " has no image");
    std::vector<Pre> pre((size_t)count);
    int max_n = 0;
    for (int b = 0; b < count; ++b) {
        std::memcpy(pre[b].KRKi, KRKi + 9 * b, sizeof(pre[b].KRKi));
        std::memcpy(pre[b].Kt, Kt + 3 * b, sizeof(pre[b].Kt));
        std::memcpy(pre[b].aff, aff + 2 * b, sizeof(pre[b].aff));
        pre[b].target = target_index[b];
        pre[b].n = h->n[first_host + b];
        if (pre[b].n > max_n) max_n = pre[b].n;
    }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->pre, pre.data(), pre.size() * sizeof(Pre), hipMemcpyHostToDevice, h->own.st));
    constexpr int per_wg = TRACE_THREADS / WAVE;
    if (max_n > 0) {
        hipLaunchKernelGGL(k_imm_trace, dim3((unsigned)((max_n + per_wg - 1) / per_wg), (unsigned)count), dim3(TRACE_THREADS), 0, h->own.st, h->points,
                           h->max_points, first_host, h->pre, h->target_c, h->target_g, h->W, h->H, h->prm);
        EDS_HIP_TRY(hipGetLastError());
    }
    std::vector<int32_t> summary;
    if (summary_out) {
        hipLaunchKernelGGL(k_imm_summary, dim3((unsigned)count), dim3(256), 0, h->own.st, h->points, h->max_points, first_host, h->pre, h->summary);
        EDS_HIP_TRY(hipGetLastError());
        summary.resize((size_t)count * edsimm::NUM_STATUS);
        EDS_HIP_TRY(hipMemcpyAsync(summary.data(), h->summary, summary.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->own.st));
    }
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    if (summary_out) std::memcpy(summary_out, summary.data(), summary.size() * sizeof(int32_t));
    return EDS_OK;
}

int eds_imm_get(eds_imm* h, int host, float* idepth_min, float* idepth_max, float* quality, int32_t* last_trace_status, float* last_trace_uv,
                float* last_trace_pixel_interval) {
    if (int rc = check_host(h, host)) return rc;
    std::vector<Point> pts;
    if (int rc = read_points(h, host, pts)) return rc;
    for (size_t i = 0; i < pts.size(); ++i) {
        const Point& p = pts[i];
        if (idepth_min) idepth_min[i] = p.idepth_min;
        if (idepth_max) idepth_max[i] = p.idepth_max;
        if (quality) quality[i] = p.quality;
        if (last_trace_status) last_trace_status[i] = p.status;
        if (last_trace_uv) { last_trace_uv[2 * i] = p.last_u; last_trace_uv[2 * i + 1] = p.last_v; }
        if (last_trace_pixel_interval) last_trace_pixel_interval[i] = p.last_interval;
    }
    return EDS_OK;
}

int eds_imm_get_points(eds_imm* h, int host, float* color, float* weights, float* gradH, float* energyTH, uint8_t* alive) {
    if (int rc = check_host(h, host)) return rc;
    std::vector<Point> pts;
    if (int rc = read_points(h, host, pts)) return rc;
    for (size_t i = 0; i < pts.size(); ++i) {
        const Point& p = pts[i];
        if (color) std::memcpy(color + 8 * i, p.color, sizeof(p.color));
        if (weights) std::memcpy(weights + 8 * i, p.weights, sizeof(p.weights));
        if (gradH) std::memcpy(gradH + 4 * i, p.gradH, sizeof(p.gradH));
        if (energyTH) energyTH[i] = p.energyTH;
        if (alive) alive[i] = (uint8_t)p.alive;
    }
    return EDS_OK;
}

int eds_imm_get_image(eds_imm* h, int which, int index, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (which != EDS_IMM_HOST_IMAGE && which != EDS_IMM_TARGET_IMAGE) return fail(EDS_ERR_INVALID, "which is EDS_IMM_HOST_IMAGE or EDS_IMM_TARGET_IMAGE");
    const bool target = which == EDS_IMM_TARGET_IMAGE;
    const int cap = target ? h->max_targets : h->max_hosts;
    if (index < 0 || index >= cap) return fail(EDS_ERR_INVALID, "frame " + std::to_string(index) + " outside 0 .. " + std::to_string(cap - 1));
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!(target ? h->target_set : h->host_set)[index]) return fail(EDS_ERR_STATE, "frame " + std::to_string(index) + " has no image");
    const size_t px = (size_t)h->W * h->H;
    std::vector<float> c(px);
    std::vector<Grad> g(px);
    if (int rc = read_back(h->own, c.data(), (target ? h->target_c : h->host_c) + px * index, px * sizeof(float))) return rc;
    if (int rc = read_back(h->own, g.data(), (target ? h->target_g : h->host_g) + px * index, px * sizeof(Grad))) return rc;
    for (size_t i = 0; i < px; ++i) { out[3 * i] = c[i]; out[3 * i + 1] = g[i].x; out[3 * i + 2] = g[i].y; }
    return EDS_OK;
}

}  // extern "C"
