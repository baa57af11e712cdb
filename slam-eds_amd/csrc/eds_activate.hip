// include/eds_hip_activate.h: activation of DSO's immature points on the device.  The arithmetic is eds_activate.hpp, shared with the
// host; this file holds the kernels and the C entry points.  Built without contraction into FMAs (csrc/Makefile).
//
// The distance map after seeding starts from an all-FAR map, so a round is one pass over the cells (k_act_round, 39 launches).  The
// candidate loop is serial by nature and runs as ONE workgroup (k_act_select, edsact::select_body): every thread takes every decision
// from the same values, thread 0 writes, and a chosen point's grow is spread over the threads one round at a time, ending at the first
// round that takes no cell.  k_act_optimize maps one wavefront to one point: lane = 8 * residual + tap, up to eight residuals per pass;
// the taps' terms are computed in parallel and the three running sums are then formed in the serial order from lane reads whose
// indices are compile-time constants, so every lane holds the same sums and the Gauss-Newton steps are one code path with the host's
// (edsact::fit_loop).  The residuals' states live in LDS (1 KB per point).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_activate.h"
#include "../../include/eds_hip_device.h"
#include "eds_activate.hpp"
#include "eds_capi_internal.hpp"
#include "eds_immature_internal.hpp"

using edsact::Calib;
using edsact::Params;
using edscapi::fail;
using edscapi::read_back;
using edsimm::Grad;
using edsimm::Point;

static_assert(sizeof(Params) == sizeof(eds_act_params), "edsact::Params is eds_act_params member for member");
static_assert(EDS_ACT_MAX_FRAMES == edsact::MAX_FRAMES && EDS_ACT_NUM_FATES == edsact::NUM_FATES, "the header's constants");

namespace {

constexpr int SELECT_THREADS = 256;

__global__ void __launch_bounds__(256) k_act_seed(uint8_t* __restrict__ map, int w1, int h1, int newest, const float* __restrict__ krki,
                                                  const float* __restrict__ kt, int n_active, const int32_t* __restrict__ active_host,
                                                  const float* __restrict__ active) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_active) return;
    const int h = active_host[i];
    if (h == newest) return;
    int u1, v1;
    float p0;
    if (edsact::map_cell(krki + 9 * h, kt + 3 * h, active[3 * i], active[3 * i + 1], active[3 * i + 2], w1, h1, &u1, &v1, &p0)) map[u1 + w1 * v1] = 0;
}

// round k in place: a cell this round writes goes from above k to k, and neither is the k - 1 a neighbour looks for
__global__ void __launch_bounds__(256) k_act_round(uint8_t* map, int w1, int h1, int k) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w1 * h1) return;
    const int x = c % w1, y = c / w1;
    if (edsact::grow_pull(map, w1, h1, k, x, y)) map[c] = (uint8_t)k;
}

struct WgSync {
    __device__ void barrier() { __syncthreads(); }
    __device__ bool any(bool b) { return __syncthreads_or(b ? 1 : 0) != 0; }
};

__global__ void __launch_bounds__(SELECT_THREADS) k_act_select(edsact::SelectIn in) {
    WgSync sync;
    edsact::select_body(in, (int)threadIdx.x, SELECT_THREADS, sync);
}

__device__ inline float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// linearizeResidual over the residuals of one point by one wavefront; every lane returns the same sums
struct WaveEval {
    const Calib& K;
    float scale_idepth, huber;
    const float* pre;                                  // the point's host's row of the precalc table
    const float* c;
    const Grad* g;
    const Point& p;
    int host, n_hosts, lane;
    int32_t *state, *new_state;
    float *energy, *new_energy;

    __device__ edsact::Sums eval(float idepth, float slack) {
        edsact::Sums a = {0.0f, 0.0f, 0.0f};
        const int n_res = n_hosts - 1, grp = lane >> 3, k = lane & 7;
        const size_t px = (size_t)K.W * K.H;
        for (int base = 0; base < n_res; base += 8) {
            const int r = base + grp;
            const bool act = r < n_res;
            const int st = act ? state[r] : (int)edsact::ST_OOB;
            const float stored = act ? energy[r] : 0.0f;
            edsact::TapOut o;
            o.fail = 1; o.e = o.h = o.b = 0.0f;
            if (act && st != edsact::ST_OOB) {
                const int t = edsact::res_target(host, r);
                const edsimm::Frame f = {c + px * t, g + px * t};
                o = edsact::tap(K, scale_idepth, huber, pre + (size_t)t * edsact::PRE_WORDS, f, p, idepth, k);
            }
            const unsigned long long fm = __ballot(o.fail != 0);
            float e = 0;
            for (int j = 0; j < 8; ++j) e += __shfl(o.e, (lane & ~7) + j);
            float ret = stored;
            if (act && st != edsact::ST_OOB && ((fm >> (8 * grp)) & 0xffull) == 0) {
                int32_t ns;
                float ne;
                edsact::verdict(e, p.energyTH, slack, &ns, &ne);
                ret = ne;
                if (k == 0) { new_state[r] = ns; new_energy[r] = ne; }
            } else if (act && k == 0) {
                new_state[r] = edsact::ST_OOB;
            }
#pragma unroll
            for (int gg = 0; gg < 8; ++gg) {
                if (base + gg >= n_res) break;
                const int stg = __builtin_amdgcn_readlane(st, gg * 8);
                if (stg != edsact::ST_OOB) {
                    const unsigned b = (unsigned)(fm >> (8 * gg)) & 0xffu;
                    const int ff = b ? __builtin_ctz(b) : 8;   // the first failing tap: what earlier taps added stays added
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (j < ff) { a.Hdd += lane_f(o.h, gg * 8 + j); a.bd += lane_f(o.b, gg * 8 + j); }
                }
                a.E = (float)((double)a.E + (double)lane_f(ret, gg * 8));
            }
        }
        __syncthreads();
        return a;
    }
    __device__ void apply() {
        if (lane < n_hosts - 1) { state[lane] = new_state[lane]; energy[lane] = new_energy[lane]; }
        __syncthreads();
    }
    __device__ int count_in() const { return __popcll(__ballot(lane < n_hosts - 1 && state[lane] == edsact::ST_IN)); }
};

// one workgroup of one wavefront per point: retires what the candidate rule deleted, fits what it chose
__global__ void __launch_bounds__(64) k_act_optimize(Point* points, int max_points, const int32_t* __restrict__ n, int n_hosts,
                                                     const float* __restrict__ pre, const float* __restrict__ host_c, const Grad* __restrict__ host_g,
                                                     Calib K, Params s, float huber, int32_t* fate, float* __restrict__ fit,
                                                     int32_t* __restrict__ res_state, float* __restrict__ res_energy, int stride) {
    __shared__ int32_t s_state[2][edsact::MAX_FRAMES];
    __shared__ float s_energy[2][edsact::MAX_FRAMES];
    const int host = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    if (i >= n[host]) return;
    const size_t idx = (size_t)host * max_points + i;
    Point* gp = points + idx;
    const int f = fate[idx];
    if (f != edsact::CHOSEN) {
        if (lane == 0 && gp->alive && edsact::leaves(f, gp->status)) gp->alive = 0;
        return;
    }
    s_state[0][lane] = s_state[1][lane] = edsact::ST_IN;
    s_energy[0][lane] = s_energy[1][lane] = 0.0f;
    __syncthreads();
    WaveEval ev = {K, s.scale_idepth, huber, pre + (size_t)host * n_hosts * edsact::PRE_WORDS, host_c, host_g, *gp, host, n_hosts, lane,
                   s_state[0], s_state[1], s_energy[0], s_energy[1]};
    const edsact::Fit o = edsact::fit_loop(ev, s, *gp);
    if (lane < n_hosts) {
        const int r = lane < host ? lane : lane - 1;
        res_state[idx * stride + lane] = lane == host ? -1 : s_state[0][r];
        res_energy[idx * stride + lane] = lane == host ? 0.0f : s_energy[0][r];
    }
    const int status = gp->status;
    __syncthreads();
    if (lane == 0) {
        fit[idx * 4] = o.idepth; fit[idx * 4 + 1] = o.E; fit[idx * 4 + 2] = o.Hdd; fit[idx * 4 + 3] = o.bd;
        fate[idx] = o.fate;
        if (edsact::leaves(o.fate, status)) gp->alive = 0;
    }
}

// the points of hosts 0 .. n_hosts - 1 per fate (integer atomics in LDS: the counts do not depend on their order); a point that just
// left the set is counted by its fate, a point that was dead before holds NONE
__global__ void __launch_bounds__(256) k_act_count(const int32_t* __restrict__ fate, int max_points, const int32_t* __restrict__ n, int n_hosts,
                                                   int32_t* __restrict__ out) {
    __shared__ int cnt[edsact::NUM_FATES];
    if (threadIdx.x < edsact::NUM_FATES) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int h = 0; h < n_hosts; ++h)
        for (int i = threadIdx.x; i < n[h]; i += blockDim.x) {
            const int f = fate[(size_t)h * max_points + i];
            if (f > 0 && f < edsact::NUM_FATES) atomicAdd(&cnt[f], 1);
        }
    __syncthreads();
    if (threadIdx.x < edsact::NUM_FATES) out[threadIdx.x] = cnt[threadIdx.x];
}

bool all_finite(const float* x, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false;
    return true;
}

// the state, allocated by the first call that needs it
int state_of(eds_imm* h, eds_act_state** out) {
    if (h->act) { *out = h->act; return EDS_OK; }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    eds_act_state* a = new eds_act_state;
    a->prm = edsact::params_default();
    a->stride = h->max_hosts < edsact::MAX_FRAMES ? h->max_hosts : edsact::MAX_FRAMES;
    const size_t cells = (size_t)(h->W >> 1) * (h->H >> 1), pts = (size_t)h->max_hosts * h->max_points, st = (size_t)a->stride;
    const size_t mark = h->own.live();
    const bool ok = h->own.alloc({{(void**)&a->map, cells},
                                  {(void**)&a->mark, cells * sizeof(uint32_t)},
                                  {(void**)&a->fate, pts * sizeof(int32_t)},
                                  {(void**)&a->fit, pts * 4 * sizeof(float)},
                                  {(void**)&a->res_state, pts * st * sizeof(int32_t)},
                                  {(void**)&a->res_energy, pts * st * sizeof(float)},
                                  {(void**)&a->krki, (size_t)h->max_hosts * 9 * sizeof(float)},
                                  {(void**)&a->kt, (size_t)h->max_hosts * 3 * sizeof(float)},
                                  {(void**)&a->pre, st * st * edsact::PRE_WORDS * sizeof(float)},
                                  {(void**)&a->n, (size_t)h->max_hosts * sizeof(int32_t)},
                                  {(void**)&a->counts, edsact::NUM_FATES * sizeof(int32_t)},
                                  {(void**)&a->flagged, (size_t)h->max_hosts}});
    if (!ok) {
        delete a;
        return fail(EDS_ERR_HIP, "eds_act: the device refused an allocation");
    }
    if (hipMemsetAsync(a->fate, 0, pts * sizeof(int32_t), h->own.st) != hipSuccess || hipStreamSynchronize(h->own.st) != hipSuccess) {
        (void)hipGetLastError();
        h->own.release_from(mark);
        delete a;
        return fail(EDS_ERR_HIP, "eds_act: the device refused a memset");
    }
    h->act = a;
    *out = a;
    return EDS_OK;
}

int check_window(const eds_imm* h, int newest, int n_hosts) {
    const int cap = h->max_hosts < edsact::MAX_FRAMES ? h->max_hosts : edsact::MAX_FRAMES;
    if (n_hosts < 1 || n_hosts > cap) return fail(EDS_ERR_INVALID, "n_hosts " + std::to_string(n_hosts) + " outside 1 .. " + std::to_string(cap));
    if (newest < 0 || newest >= n_hosts) return fail(EDS_ERR_INVALID, "newest " + std::to_string(newest) + " outside 0 .. " + std::to_string(n_hosts - 1));
    return EDS_OK;
}

int upload_counts(eds_imm* h, eds_act_state* a, int n_hosts) {
    std::vector<int32_t> n(h->n.begin(), h->n.begin() + n_hosts);
    EDS_HIP_TRY(hipMemcpyAsync(a->n, n.data(), n.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));       // n is a local
    return EDS_OK;
}

int read_counts(eds_imm* h, eds_act_state* a, int n_hosts, int32_t* counts_out) {
    hipLaunchKernelGGL(k_act_count, dim3(1), dim3(256), 0, h->own.st, a->fate, h->max_points, a->n, n_hosts, a->counts);
    EDS_HIP_TRY(hipGetLastError());
    int32_t c[edsact::NUM_FATES];
    if (int rc = read_back(h->own, c, a->counts, sizeof(c))) return rc;
    if (counts_out) std::memcpy(counts_out, c, sizeof(c));
    return EDS_OK;
}

}  // namespace

namespace edsimm_internal {
void act_release(eds_imm* h) {
    delete h->act;
    h->act = nullptr;
}
void act_invalidate(eds_imm* h) {
    if (h->act) h->act->map_valid = h->act->sel_valid = h->act->fit_valid = false;
}
}  // namespace edsimm_internal

extern "C" {

int eds_act_abi_version(void) { return EDS_HIP_ACTIVATE_ABI_VERSION; }

void eds_act_params_default(eds_act_params* p) {
    if (!p) return;
    const Params d = edsact::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_act_set_params(eds_imm* h, const eds_act_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null parameters");
    Params s;
    std::memcpy(&s, p, sizeof(s));
    if (!edsact::params_valid(s))
        return fail(EDS_ERR_INVALID, "parameters: every float finite; scale_idepth > 0; gn_its_on_point_activation 0 .. 16; min_obs 0 .. 64");
    eds_act_state* a;
    if (int rc = state_of(h, &a)) return rc;
    a->prm = s;
    return EDS_OK;
}

int eds_act_get_params(eds_imm* h, eds_act_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null output");
    const Params s = h->act ? h->act->prm : edsact::params_default();
    std::memcpy(p, &s, sizeof(s));
    return EDS_OK;
}

int eds_act_set_calib(eds_imm* h, float fx, float fy, float cx, float cy) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!edscapi::check_calib(fx, fy, cx, cy)) return fail(EDS_ERR_INVALID, "calibration: fx, fy finite and positive, cx, cy finite");
    if ((h->W >> 1) < 3 || (h->H >> 1) < 3) return fail(EDS_ERR_INVALID, "the level-1 map is at least 3 x 3");
    eds_act_state* a;
    if (int rc = state_of(h, &a)) return rc;
    a->cal = edsact::make_calib(h->H, h->W, fx, fy, cx, cy);
    a->calib_set = true;
    a->map_valid = a->sel_valid = a->fit_valid = false;
    return EDS_OK;
}

int eds_act_make_distance_map(eds_imm* h, int newest, int n_hosts, const float* KRKi1, const float* Kt1, int n_active, const int32_t* active_host,
                              const float* active, int on_device) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (int rc = check_window(h, newest, n_hosts)) return rc;
    if (!KRKi1 || !Kt1) return fail(EDS_ERR_INVALID, "KRKi1 and Kt1 are required");
    if (n_active < 0 || n_active > (1 << 26)) return fail(EDS_ERR_INVALID, "n_active is 0 .. 2^26");
    if (n_active > 0 && (!active_host || !active)) return fail(EDS_ERR_INVALID, "active_host and active_uv_idepth are required");
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    if (!all_finite(KRKi1, 9 * (size_t)n_hosts) || !all_finite(Kt1, 3 * (size_t)n_hosts)) return fail(EDS_ERR_INVALID, "KRKi1 or Kt1 is not finite");
    if (!h->act || !h->act->calib_set) return fail(EDS_ERR_STATE, "eds_act_set_calib first");
    eds_act_state* a = h->act;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    std::vector<int32_t> hosts((size_t)n_active);
    if (n_active > 0) {
        if (on_device) {
            if (reinterpret_cast<uintptr_t>(active_host) % 4 || reinterpret_cast<uintptr_t>(active) % 4) return fail(EDS_ERR_INVALID, "active points: not aligned to 4 bytes");
            if (int rc = eds_dev_check_range(h->own.dev, active_host, (size_t)n_active * sizeof(int32_t))) return rc;
            if (int rc = eds_dev_check_range(h->own.dev, active, (size_t)n_active * 3 * sizeof(float))) return rc;
            if (int rc = read_back(h->own, hosts.data(), active_host, hosts.size() * sizeof(int32_t))) return rc;
        } else {
            std::memcpy(hosts.data(), active_host, hosts.size() * sizeof(int32_t));
        }
        std::vector<uint8_t> seen((size_t)n_hosts, 0);
        for (int i = 0; i < n_active; ++i) {
            const int hh = hosts[i];
            if (hh < 0 || hh >= n_hosts) return fail(EDS_ERR_INVALID, "active point " + std::to_string(i) + ": host " + std::to_string(hh) + " outside the window");
            if (i > 0 && hosts[i - 1] != hh && seen[hh]) return fail(EDS_ERR_INVALID, "the active points are not grouped by host");
            seen[hh] = 1;
        }
        if (!on_device) {
            if (n_active > a->active_cap) {
                h->own.release(a->active);
                h->own.release(a->active_host);
                a->active_cap = 0;
                if (!h->own.alloc({{(void**)&a->active, (size_t)n_active * 3 * sizeof(float)}, {(void**)&a->active_host, (size_t)n_active * sizeof(int32_t)}}))
                    return fail(EDS_ERR_HIP, "eds_act_make_distance_map: the device refused an allocation");
                a->active_cap = n_active;
            }
            EDS_HIP_TRY(hipMemcpyAsync(a->active, active, (size_t)n_active * 3 * sizeof(float), hipMemcpyHostToDevice, h->own.st));
            EDS_HIP_TRY(hipMemcpyAsync(a->active_host, hosts.data(), hosts.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
            active = a->active;
            active_host = a->active_host;
        }
    }
    const int w1 = a->cal.w1, h1 = a->cal.h1, cells = w1 * h1;
    a->map_valid = a->sel_valid = false;
    EDS_HIP_TRY(hipMemcpyAsync(a->krki, KRKi1, 9 * (size_t)n_hosts * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(a->kt, Kt1, 3 * (size_t)n_hosts * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(a->map, edsact::FAR, (size_t)cells, h->own.st));
    if (n_active > 0) {
        hipLaunchKernelGGL(k_act_seed, dim3((unsigned)((n_active + 255) / 256)), dim3(256), 0, h->own.st, a->map, w1, h1, newest, a->krki, a->kt, n_active,
                           active_host, active);
        EDS_HIP_TRY(hipGetLastError());
        for (int k = 1; k <= edsact::ROUNDS; ++k) hipLaunchKernelGGL(k_act_round, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->own.st, a->map, w1, h1, k);
        EDS_HIP_TRY(hipGetLastError());
    }
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    a->map_valid = true;
    return EDS_OK;
}

int eds_act_get_distance_map(eds_imm* h, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->act || !h->act->map_valid) return fail(EDS_ERR_STATE, "no distance map: eds_act_make_distance_map first");
    const size_t cells = (size_t)h->act->cal.w1 * h->act->cal.h1;
    std::vector<uint8_t> m(cells);
    if (int rc = read_back(h->own, m.data(), h->act->map, cells)) return rc;
    for (size_t i = 0; i < cells; ++i) out[i] = edsact::map_value(m[i]);
    return EDS_OK;
}

int eds_act_select(eds_imm* h, int newest, int n_hosts, const float* KRKi1, const float* Kt1, const uint8_t* flagged, float current_min_act_dist,
                   int32_t* counts_out) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (int rc = check_window(h, newest, n_hosts)) return rc;
    if (!KRKi1 || !Kt1) return fail(EDS_ERR_INVALID, "KRKi1 and Kt1 are required");
    if (!all_finite(KRKi1, 9 * (size_t)n_hosts) || !all_finite(Kt1, 3 * (size_t)n_hosts) || !std::isfinite(current_min_act_dist))
        return fail(EDS_ERR_INVALID, "KRKi1, Kt1 or current_min_act_dist is not finite");
    if (!h->act || !h->act->calib_set) return fail(EDS_ERR_STATE, "eds_act_set_calib first");
    eds_act_state* a = h->act;
    if (!a->map_valid) return fail(EDS_ERR_STATE, "no distance map: eds_act_make_distance_map first");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    std::vector<uint8_t> fl((size_t)n_hosts, 0);
    if (flagged) for (int i = 0; i < n_hosts; ++i) fl[i] = flagged[i] ? 1 : 0;
    a->sel_valid = a->fit_valid = false;
    EDS_HIP_TRY(hipMemcpyAsync(a->krki, KRKi1, 9 * (size_t)n_hosts * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(a->kt, Kt1, 3 * (size_t)n_hosts * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(a->flagged, fl.data(), fl.size(), hipMemcpyHostToDevice, h->own.st));
    if (int rc = upload_counts(h, a, n_hosts)) return rc;
    edsact::SelectIn in = {h->points, h->max_points, a->n, newest, n_hosts, a->krki, a->kt, a->flagged, current_min_act_dist, a->prm, a->cal.w1, a->cal.h1,
                           a->map, a->mark, a->fate, a->counts};
    hipLaunchKernelGGL(k_act_select, dim3(1), dim3(SELECT_THREADS), 0, h->own.st, in);
    EDS_HIP_TRY(hipGetLastError());
    int32_t c[edsact::NUM_FATES];
    if (int rc = read_back(h->own, c, a->counts, sizeof(c))) return rc;
    if (counts_out) std::memcpy(counts_out, c, sizeof(c));
    a->sel_valid = true;
    a->sel_hosts = n_hosts;
    return EDS_OK;
}

int eds_act_optimize(eds_imm* h, int n_hosts, const float* precalc, int32_t* counts_out) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!precalc) return fail(EDS_ERR_INVALID, "precalc is required");
    if (!h->act || !h->act->sel_valid) return fail(EDS_ERR_STATE, "no selection: eds_act_select first");
    eds_act_state* a = h->act;
    if (n_hosts != a->sel_hosts) return fail(EDS_ERR_INVALID, "n_hosts " + std::to_string(n_hosts) + " is not the selection's " + std::to_string(a->sel_hosts));
    for (int i = 0; i < n_hosts; ++i)
        for (int j = 0; j < n_hosts; ++j)
            if (i != j && !all_finite(precalc + (size_t)(i * n_hosts + j) * edsact::PRE_WORDS, edsact::PRE_WORDS)) return fail(EDS_ERR_INVALID, "precalc is not finite");
    for (int i = 0; i < n_hosts; ++i)
        if (!h->host_set[i]) return fail(EDS_ERR_STATE, "frame " + std::to_string(i) + " has no image");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    a->sel_valid = false;
    EDS_HIP_TRY(hipMemcpyAsync(a->pre, precalc, (size_t)n_hosts * n_hosts * edsact::PRE_WORDS * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    int max_n = 0;
    for (int i = 0; i < n_hosts; ++i) if (h->n[i] > max_n) max_n = h->n[i];
    if (max_n > 0) {
        hipLaunchKernelGGL(k_act_optimize, dim3((unsigned)max_n, (unsigned)n_hosts), dim3(64), 0, h->own.st, h->points, h->max_points, a->n, n_hosts, a->pre,
                           h->host_c, h->host_g, a->cal, a->prm, h->prm.huber_th, a->fate, a->fit, a->res_state, a->res_energy, a->stride);
        EDS_HIP_TRY(hipGetLastError());
    }
    if (int rc = read_counts(h, a, n_hosts, counts_out)) return rc;
    a->fit_valid = true;
    return EDS_OK;
}

int eds_act_get(eds_imm* h, int host, int32_t* fate, float* idepth, float* energy, float* hdd, float* bd, int32_t* res_state, float* res_energy) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (host < 0 || host >= h->max_hosts) return fail(EDS_ERR_INVALID, "host " + std::to_string(host) + " outside 0 .. " + std::to_string(h->max_hosts - 1));
    if (!h->act || !(h->act->sel_valid || h->act->fit_valid)) return fail(EDS_ERR_STATE, "no selection: eds_act_select first");
    eds_act_state* a = h->act;
    const int F = a->sel_hosts;
    if (host >= F) return fail(EDS_ERR_INVALID, "host " + std::to_string(host) + " is not in the selection's window");
    const size_t n = (size_t)h->n[host], st = (size_t)a->stride, o = (size_t)host * h->max_points;
    if (n == 0) return EDS_OK;
    std::vector<int32_t> f(n), rs(n * st);
    std::vector<float> ft(n * 4), re(n * st);
    if (int rc = read_back(h->own, f.data(), a->fate + o, n * sizeof(int32_t))) return rc;
    if (int rc = read_back(h->own, ft.data(), a->fit + o * 4, n * 4 * sizeof(float))) return rc;
    if (int rc = read_back(h->own, rs.data(), a->res_state + o * st, n * st * sizeof(int32_t))) return rc;
    if (int rc = read_back(h->own, re.data(), a->res_energy + o * st, n * st * sizeof(float))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const bool fitted = f[i] == edsact::KEPT_WEAK || f[i] == edsact::DROPPED || f[i] == edsact::ACTIVATED;
        if (fate) fate[i] = f[i];
        if (idepth) idepth[i] = fitted ? ft[4 * i] : 0.0f;
        if (energy) energy[i] = fitted ? ft[4 * i + 1] : 0.0f;
        if (hdd) hdd[i] = fitted ? ft[4 * i + 2] : 0.0f;
        if (bd) bd[i] = fitted ? ft[4 * i + 3] : 0.0f;
        for (int t = 0; t < F; ++t) {
            if (res_state) res_state[i * F + t] = fitted ? rs[i * st + t] : -1;
            if (res_energy) res_energy[i * F + t] = fitted ? re[i * st + t] : 0.0f;
        }
    }
    return EDS_OK;
}

int eds_act_get_activated(eds_imm* h, int cap, int* n_out, int32_t* host, int32_t* index, float* uv, float* type, float* idepth, float* color,
                          float* weights, uint64_t* target_mask) {
    if (int rc = edscapi::check_handle(h, "eds_imm")) return rc;
    if (!n_out || cap < 0) return fail(EDS_ERR_INVALID, "n is required and cap is not negative");
    if (!h->act || !h->act->fit_valid) return fail(EDS_ERR_STATE, "no fit: eds_act_optimize first");
    eds_act_state* a = h->act;
    const int F = a->sel_hosts;
    const size_t st = (size_t)a->stride;
    int m = 0;
    for (int hh = 0; hh < F; ++hh) {
        const size_t n = (size_t)h->n[hh], o = (size_t)hh * h->max_points;
        if (n == 0) continue;
        std::vector<int32_t> f(n), rs(n * st);
        std::vector<float> ft(n * 4);
        std::vector<Point> pts(n);
        if (int rc = read_back(h->own, f.data(), a->fate + o, n * sizeof(int32_t))) return rc;
        if (int rc = read_back(h->own, ft.data(), a->fit + o * 4, n * 4 * sizeof(float))) return rc;
        if (int rc = read_back(h->own, rs.data(), a->res_state + o * st, n * st * sizeof(int32_t))) return rc;
        if (int rc = read_back(h->own, pts.data(), h->points + o, n * sizeof(Point))) return rc;
        for (size_t i = 0; i < n; ++i) {
            if (f[i] != edsact::ACTIVATED) continue;
            if (m < cap) {
                const Point& p = pts[i];
                if (host) host[m] = hh;
                if (index) index[m] = (int32_t)i;
                if (uv) { uv[2 * m] = p.u; uv[2 * m + 1] = p.v; }
                if (type) type[m] = p.type;
                if (idepth) idepth[m] = ft[4 * i] * a->prm.scale_idepth;
                if (color) std::memcpy(color + 8 * (size_t)m, p.color, sizeof(p.color));
                if (weights) std::memcpy(weights + 8 * (size_t)m, p.weights, sizeof(p.weights));
                if (target_mask) {
                    uint64_t mask = 0;
                    for (int t = 0; t < F; ++t) if (rs[i * st + t] == edsact::ST_IN) mask |= (uint64_t)1 << t;
                    target_mask[m] = mask;
                }
            }
            ++m;
        }
    }
    *n_out = m;
    return EDS_OK;
}

}  // extern "C"
