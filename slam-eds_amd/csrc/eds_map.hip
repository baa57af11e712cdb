// The map as a point cloud and as the next keyframe's depth map, on the device (include/eds_hip_map.h), from the tables an eds_win, an
// eds_imm and an eds_trk already hold:
//
//   k_map_window_cloud   dso::io::getMap (reference src/io/OutputMaps.cpp:38-91): a plain map, one lane per selected point, one or eight
//                        world points each; a point's place comes from its host's run and the selected hosts' output bases.
//   k_map_depth          the single-point cloud -> T_dst_w -> IDepthMap::fromPoints (src/mapping/Types.hpp:248-275): one workgroup per
//                        destination map walks the selected hosts' runs in sweeps of edsmap::CHUNK points; a ballot and the count of the
//                        lower lanes rank a kept point inside its wavefront, the wavefronts' totals come from LDS, a running base goes
//                        from sweep to sweep: a stable scatter, one pass.
//   k_map_immature       getImmatureMap (:93-148): one workgroup; it counts the cloud first (a too-small cap is answered with the count
//                        and nothing else is written), then compacts the same way.
//   k_map_slot_cloud     KeyFrame::getMap's points (src/tracking/KeyFrame.cpp:1244-1300) of tracker slots.
//
// The arithmetic is edsmap:: (eds_map.hpp), shared with the host; this translation unit is compiled with -ffp-contract=off (Makefile).
// Runs, masks, calibration and the hosts' poses travel as kernel arguments; the destinations' poses and the counts sit in a pinned,
// device-mapped block, so a call is one launch and one wait for the stream, after which its counts are on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/eds_hip_map.h"
#include "eds_capi_internal.hpp"
#include "eds_immature_internal.hpp"
#include "eds_map.hpp"
#include "eds_window_internal.hpp"

using namespace edscapi;

// the scratch of one handle: a pinned, device-mapped block (poses of the destinations, counts) and device memory for results that go to
// host memory.  Both belong to the handle's owner.
struct eds_map_state {
    char *h_pin = nullptr, *d_pin = nullptr;
    size_t pin_bytes = 0;
    char* stage = nullptr;
    size_t stage_bytes = 0;
};

namespace edsmap_internal {
void release(eds_map_state*& s) {
    delete s;
    s = nullptr;
}
}  // namespace edsmap_internal

namespace {

constexpr int TB = 256;
constexpr int CT = edsmap::CHUNK;
constexpr int SLOT_BATCH = 16;                                  // slots per launch of k_map_slot_cloud: their poses are kernel arguments

struct WinArgs {
    int32_t first[edsmap::MAX_FRAMES + 1];
    int32_t obase[edsmap::MAX_FRAMES + 1];                      // selected points before host h; [F ..]: all of them
    uint32_t mask;
    int32_t F, fan, nsel;
    edsmap::Calib cal;
    double T[12 * edsmap::MAX_FRAMES];
};

__global__ __launch_bounds__(TB) void k_map_window_cloud(WinArgs a, const edswin::Point* __restrict__ pts, const float* __restrict__ ids,
                                                         double* __restrict__ out) {
    __shared__ double s_T[12 * edsmap::MAX_FRAMES];
    for (int i = threadIdx.x; i < 12 * a.F; i += TB) s_T[i] = a.T[i];
    __syncthreads();
    const int j = blockIdx.x * TB + threadIdx.x;
    if (j >= a.nsel) return;
    int h = 0;
    for (int f = 0; f < a.F; ++f)
        if (j >= a.obase[f] && j < a.obase[f + 1]) h = f;
    const int p = a.first[h] + (j - a.obase[h]);
    const float u = pts[p].u, v = pts[p].v, id = ids[p];
    double* o = out + (size_t)j * a.fan * 3;
#pragma unroll
    for (int k = 0; k < edsmap::FAN; ++k) {
        if (k >= a.fan) break;
        double w[3];
        edsmap::window_point(a.cal, s_T + 12 * h, u, v, id, k, w);
        o[3 * k] = w[0]; o[3 * k + 1] = w[1]; o[3 * k + 2] = w[2];
    }
}

struct DepthArgs {
    int32_t first[edsmap::MAX_FRAMES + 1];
    uint32_t mask;
    int32_t F;
    edsmap::Calib cal;
    double dW, dH;
    long long stride;
    double T[12 * edsmap::MAX_FRAMES];
};

// map b = blockIdx.x: par + 16 b holds T_dst_w (12) and K_dst (4); n_out[b], and xy / idp / src from b * stride
__global__ __launch_bounds__(CT) void k_map_depth(DepthArgs a, const edswin::Point* __restrict__ pts, const float* __restrict__ ids,
                                                  const double* __restrict__ par, int* __restrict__ n_out, double* __restrict__ xy,
                                                  double* __restrict__ idp, int32_t* __restrict__ src) {
    __shared__ double s_T[12 * edsmap::MAX_FRAMES], s_par[16];
    __shared__ int s_wave[CT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 12 * a.F) s_T[tid] = a.T[tid];
    if (tid >= 128 && tid < 144) s_par[tid - 128] = par[(size_t)b * 16 + (tid - 128)];
    __syncthreads();
    const size_t ob = (size_t)b * (size_t)a.stride;
    int run = 0;
    for (int h = 0; h < a.F; ++h) {
        if (!((a.mask >> h) & 1u)) continue;
        const int p1 = a.first[h + 1];
        for (int c0 = a.first[h]; c0 < p1; c0 += CT) {
            const int p = c0 + tid;
            bool keep = false;
            double px = 0.0, py = 0.0, ip = 0.0;
            if (p < p1) {
                double w[3], d[3];
                edsmap::window_point(a.cal, s_T + 12 * h, pts[p].u, pts[p].v, ids[p], 0, w);
                edsmap::transform(s_par, w, d);
                keep = edsmap::project(s_par + 12, a.dW, a.dH, d, &px, &py, &ip);
            }
            int total;
            const int rank = edsdso::block_rank<CT>(keep, s_wave, &total);
            if (keep) {
                const size_t dst = ob + (size_t)(run + rank);
                xy[2 * dst] = px; xy[2 * dst + 1] = py;
                idp[dst] = ip;
                if (src) src[dst] = p;
            }
            run += total;
        }
    }
    if (tid == 0) n_out[b] = run;
}

struct ImmArgs {
    int32_t n[edsmap::MAX_IMM_HOSTS];
    uint32_t mask;
    int32_t n_hosts, pitch, fan;
    long long cap;
    edsmap::Calib cal;
};

// n_out[0]: the entries the cloud has, n_out[1]: 1 when they were written (cap held them)
__global__ __launch_bounds__(CT) void k_map_immature(ImmArgs a, const edsimm::Point* __restrict__ pts, const double* __restrict__ par,
                                                     int* __restrict__ n_out, double* __restrict__ points, double* __restrict__ colors,
                                                     uint8_t* __restrict__ status) {
    __shared__ double s_T[12 * edsmap::MAX_IMM_HOSTS];
    __shared__ int s_wave[CT / 64];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    if (tid < 12 * a.n_hosts) s_T[tid] = par[tid];
    if (tid == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int h = 0; h < a.n_hosts; ++h) {
        if (!((a.mask >> h) & 1u)) continue;
        const edsimm::Point* __restrict__ row = pts + (size_t)h * a.pitch;
        for (int p = tid; p < a.n[h]; p += CT) {
            double d;
            mine += edsmap::immature_depth(row[p].alive, row[p].idepth_min, row[p].idepth_max, &d) ? 1 : 0;
        }
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    const long long needed = (long long)s_count * a.fan;
    if (needed > a.cap) {
        if (tid == 0) { n_out[0] = (int)needed; n_out[1] = 0; }
        return;
    }
    int run = 0;
    for (int h = 0; h < a.n_hosts; ++h) {
        if (!((a.mask >> h) & 1u)) continue;
        const edsimm::Point* __restrict__ row = pts + (size_t)h * a.pitch;
        const int nh = a.n[h];
        for (int c0 = 0; c0 < nh; c0 += CT) {
            const int p = c0 + tid;
            bool keep = false;
            double d = 0.0;
            float u = 0.0f, v = 0.0f;
            int32_t st = 0;
            if (p < nh) {
                keep = edsmap::immature_depth(row[p].alive, row[p].idepth_min, row[p].idepth_max, &d);
                u = row[p].u; v = row[p].v; st = row[p].status;
            }
            int total;
            const int rank = edsdso::block_rank<CT>(keep, s_wave, &total);
            if (keep) {
                const size_t q0 = (size_t)(run + rank) * a.fan;
                double col[4];
                edsmap::status_color(st, col);
#pragma unroll
                for (int k = 0; k < edsmap::FAN; ++k) {
                    if (k >= a.fan) break;
                    double P[3], w[3];
                    edsmap::back_project(a.cal, u, v, d, k, P);
                    edsmap::transform(s_T + 12 * h, P, w);
                    const size_t q = q0 + k;
                    points[3 * q] = w[0]; points[3 * q + 1] = w[1]; points[3 * q + 2] = w[2];
                    if (colors) { colors[4 * q] = col[0]; colors[4 * q + 1] = col[1]; colors[4 * q + 2] = col[2]; colors[4 * q + 3] = col[3]; }
                    if (status) status[q] = (uint8_t)st;
                }
            }
            run += total;
        }
    }
    if (tid == 0) { n_out[0] = run * a.fan; n_out[1] = 1; }
}

struct SlotArgs {
    int32_t seeded[SLOT_BATCH];
    double T[12 * SLOT_BATCH];
};

// point i = blockIdx.x * TB + lane of slot first + blockIdx.y, written at (blockIdx.y * stride + i) of out
__global__ __launch_bounds__(TB) void k_map_slot_cloud(EdsArrays A, SlotArgs a, int first, const double* __restrict__ seeds_mu, long long stride,
                                                       double* __restrict__ out) {
    __shared__ double s_T[12];
    const int b = blockIdx.y, slot = first + b, i = blockIdx.x * TB + threadIdx.x;
    if (threadIdx.x < 12) s_T[threadIdx.x] = a.T[12 * b + threadIdx.x];
    __syncthreads();
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    if (i >= N || i >= stride) return;
    const size_t o = (size_t)slot * A.Np + i;
    const double mu = a.seeded[b] ? seeds_mu[o] : (double)A.rho[o];
    double w[3];
    edsmap::slot_point(s_T, (double)A.x[o], (double)A.y[o], mu, w);
    double* dst = out + ((size_t)b * (size_t)stride + i) * 3;
    dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the state with a pinned block of at least pin_bytes and device scratch of at least stage_bytes, both the owner's
int ensure_state(eds_map_state*& s, DeviceOwner& own, size_t pin_bytes, size_t stage_bytes) {
    if (!s) s = new eds_map_state;
    const size_t want = std::max<size_t>(pin_bytes, 4096);
    if (pin_bytes > s->pin_bytes && !own.regrow(s->pin_bytes, want, {mapped(s->h_pin, s->d_pin, want)}))
        return fail(EDS_ERR_HIP, "eds_map: allocation of the pinned block failed");
    if (stage_bytes > s->stage_bytes && !own.regrow(s->stage_bytes, stage_bytes, {{(void**)&s->stage, stage_bytes}}))
        return fail(EDS_ERR_HIP, "eds_map: allocation of the device scratch failed");
    return EDS_OK;
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

int check_flag(int v, const char* name) { return v == 0 || v == 1 ? (int)EDS_OK : fail(EDS_ERR_INVALID, std::string(name) + " is 0 or 1"); }

// what both eds_map_window_* calls check of the window, and the runs of its hosts
int window_runs(eds_win* h, int F, uint32_t mask, const double* T_w_c, edsmap::Runs* runs, int32_t* per_host, int* nsel) {
    if (int rc = check_handle(h, "eds_win")) return rc;
    if (F < 1 || F > edsmap::MAX_FRAMES) return fail(EDS_ERR_INVALID, "F is 1 .. 8");
    if (!T_w_c) return fail(EDS_ERR_INVALID, "null T_w_c");
    if (!edsmap::finite_all(T_w_c, 12 * (int64_t)F)) return fail(EDS_ERR_INVALID, "T_w_c is not finite");
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_win_set_calib has not been called");
    if (!edsmap::make_runs(h->n, h->host_of.data(), F, runs))
        return fail(EDS_ERR_INVALID, "a point is hosted by a frame at or above F, or the points are not in nondecreasing host order");
    *nsel = edsmap::selected_points(*runs, F, mask, per_host);
    return EDS_OK;
}

edsmap::Calib calib_of(const eds_win* h) { edsmap::Calib c = {h->cal.fx, h->cal.fy, h->cal.cx, h->cal.cy}; return c; }

}  // namespace

extern "C" {

int eds_map_abi_version(void) { return EDS_HIP_MAP_ABI_VERSION; }

int eds_map_window_cloud(eds_win* h, int F, uint32_t frame_mask, const double* T_w_c, int single_point, double* points, int on_device,
                         int32_t* n_out, int32_t* per_host) {
    edsmap::Runs runs;
    int32_t per[edsmap::MAX_FRAMES];
    int nsel = 0, rc;
    if ((rc = window_runs(h, F, frame_mask, T_w_c, &runs, per, &nsel))) return rc;
    if ((rc = check_flag(single_point, "single_point")) || (rc = check_flag(on_device, "on_device"))) return rc;
    if (!n_out) return fail(EDS_ERR_INVALID, "null n_out");
    const int fan = single_point ? 1 : edsmap::FAN;
    const size_t total = (size_t)nsel * fan, bytes = total * 3 * sizeof(double);
    if (total && !points) return fail(EDS_ERR_INVALID, "null points");
    if (total && on_device && (rc = eds_dev_check_range(h->own.dev, points, bytes))) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (total) {
        if (!on_device && (rc = ensure_state(h->map, h->own, 0, bytes))) return rc;
        WinArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int f = 0, q = 0; f <= edsmap::MAX_FRAMES; ++f) {
            a.first[f] = runs.first[f];
            a.obase[f] = q;
            if (f < edsmap::MAX_FRAMES) q += per[f];
        }
        a.mask = frame_mask; a.F = F; a.fan = fan; a.nsel = nsel; a.cal = calib_of(h);
        std::memcpy(a.T, T_w_c, 12 * (size_t)F * sizeof(double));
        double* dst = on_device ? points : reinterpret_cast<double*>(h->map->stage);
        hipLaunchKernelGGL(k_map_window_cloud, dim3(blocks(nsel, TB)), dim3(TB), 0, h->own.st, a, h->pts, h->ids, dst);
        EDS_HIP_TRY(hipGetLastError());
        if (!on_device) EDS_HIP_TRY(hipMemcpyAsync(points, dst, bytes, hipMemcpyDeviceToHost, h->own.st));
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    }
    *n_out = (int32_t)total;
    if (per_host) std::memcpy(per_host, per, sizeof(per));
    return EDS_OK;
}

int eds_map_window_depth_maps(eds_win* h, int F, uint32_t frame_mask, const double* T_w_c, int count, const double* T_dst_w,
                              const double* K_dst, int dst_H, int dst_W, int64_t stride, double* depth_xy, double* depth_idp,
                              int32_t* src_index, int on_device, int32_t* n_out) {
    edsmap::Runs runs;
    int nsel = 0, rc;
    if ((rc = window_runs(h, F, frame_mask, T_w_c, &runs, nullptr, &nsel))) return rc;
    if ((rc = check_flag(on_device, "on_device"))) return rc;
    if (count < 1 || count > (1 << 16)) return fail(EDS_ERR_INVALID, "count is 1 .. 65536");
    if (!T_dst_w || !K_dst || !n_out || !depth_xy || !depth_idp) return fail(EDS_ERR_INVALID, "null T_dst_w, K_dst, depth_xy, depth_idp or n_out");
    if (dst_H < 1 || dst_W < 1) return fail(EDS_ERR_INVALID, "dst_H and dst_W are at least 1");
    if (!edsmap::finite_all(T_dst_w, 12 * (int64_t)count)) return fail(EDS_ERR_INVALID, "T_dst_w is not finite");
    if (!edsmap::finite_all(K_dst, 4 * (int64_t)count)) return fail(EDS_ERR_INVALID, "K_dst is not finite");
    for (int b = 0; b < count; ++b)
        if (K_dst[4 * (size_t)b] == 0.0 || K_dst[4 * (size_t)b + 1] == 0.0) return fail(EDS_ERR_INVALID, "K_dst has a zero focal length");
    if (stride < nsel || stride > ((int64_t)1 << 40)) return fail(EDS_ERR_INVALID, "stride smaller than the selected hosts' points");
    const size_t extent = nsel ? (size_t)(count - 1) * (size_t)stride + (size_t)nsel : 0;
    if (on_device && extent) {
        if ((rc = eds_dev_check_range(h->own.dev, depth_xy, extent * 16)) || (rc = eds_dev_check_range(h->own.dev, depth_idp, extent * 8))) return rc;
        if (src_index && (rc = eds_dev_check_range(h->own.dev, src_index, extent * 4))) return rc;
    }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t par_bytes = (size_t)count * 16 * sizeof(double), cells = (size_t)count * (size_t)nsel;
    const size_t o_idp = round16(cells * 16), o_src = o_idp + round16(cells * 8);
    if ((rc = ensure_state(h->map, h->own, par_bytes + (size_t)count * sizeof(int), on_device || !cells ? 0 : o_src + cells * 4))) return rc;
    eds_map_state* s = h->map;
    double* h_par = reinterpret_cast<double*>(s->h_pin);
    int* h_n = reinterpret_cast<int*>(s->h_pin + par_bytes);
    for (int b = 0; b < count; ++b) {
        std::memcpy(h_par + 16 * (size_t)b, T_dst_w + 12 * (size_t)b, 12 * sizeof(double));
        std::memcpy(h_par + 16 * (size_t)b + 12, K_dst + 4 * (size_t)b, 4 * sizeof(double));
        h_n[b] = 0;
    }
    if (nsel) {
        DepthArgs a;
        std::memset(&a, 0, sizeof(a));
        std::memcpy(a.first, runs.first, sizeof(a.first));
        a.mask = frame_mask; a.F = F; a.cal = calib_of(h); a.dW = (double)dst_W; a.dH = (double)dst_H;
        a.stride = on_device ? (long long)stride : (long long)nsel;
        std::memcpy(a.T, T_w_c, 12 * (size_t)F * sizeof(double));
        double *d_xy = depth_xy, *d_idp = depth_idp;
        int32_t* d_src = src_index;
        if (!on_device) {
            d_xy = reinterpret_cast<double*>(s->stage);
            d_idp = reinterpret_cast<double*>(s->stage + o_idp);
            d_src = src_index ? reinterpret_cast<int32_t*>(s->stage + o_src) : nullptr;
        }
        hipLaunchKernelGGL(k_map_depth, dim3(count), dim3(CT), 0, h->own.st, a, h->pts, h->ids, reinterpret_cast<const double*>(s->d_pin),
                           reinterpret_cast<int*>(s->d_pin + par_bytes), d_xy, d_idp, d_src);
        EDS_HIP_TRY(hipGetLastError());
        std::vector<char> back;
        if (!on_device) {
            back.resize(o_src + (src_index ? cells * 4 : 0));
            EDS_HIP_TRY(hipMemcpyAsync(back.data(), s->stage, back.size(), hipMemcpyDeviceToHost, h->own.st));
        }
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
        if (!on_device)
            for (int b = 0; b < count; ++b) {
                const size_t n = (size_t)h_n[b], from = (size_t)b * nsel, to = (size_t)b * (size_t)stride;
                std::memcpy(depth_xy + 2 * to, back.data() + from * 16, n * 16);
                std::memcpy(depth_idp + to, back.data() + o_idp + from * 8, n * 8);
                if (src_index) std::memcpy(src_index + to, back.data() + o_src + from * 4, n * 4);
            }
    }
    for (int b = 0; b < count; ++b) n_out[b] = h_n[b];
    return EDS_OK;
}

int eds_map_immature_cloud(eds_imm* h, int n_hosts, uint32_t host_mask, const double* T_w_c, const float calib[4], int single_point,
                           int64_t cap, double* points, double* colors, uint8_t* status, int on_device, int32_t* n_out) {
    int rc;
    if ((rc = check_handle(h, "eds_imm"))) return rc;
    if (n_hosts < 1 || n_hosts > edsmap::MAX_IMM_HOSTS || n_hosts > h->max_hosts) return fail(EDS_ERR_INVALID, "n_hosts is 1 .. min(32, max_hosts)");
    if (!T_w_c || !calib || !n_out) return fail(EDS_ERR_INVALID, "null T_w_c, calib or n_out");
    if (!edsmap::finite_all(T_w_c, 12 * (int64_t)n_hosts)) return fail(EDS_ERR_INVALID, "T_w_c is not finite");
    if (!check_calib(calib[0], calib[1], calib[2], calib[3])) return fail(EDS_ERR_INVALID, "calib is not finite, or a focal length is not positive");
    if ((rc = check_flag(single_point, "single_point")) || (rc = check_flag(on_device, "on_device"))) return rc;
    if (cap < 0) return fail(EDS_ERR_INVALID, "negative cap");
    const int fan = single_point ? 1 : edsmap::FAN;
    ImmArgs a;
    std::memset(&a, 0, sizeof(a));
    int64_t most = 0;                                           // the cloud's size were every selected point kept
    for (int f = 0; f < n_hosts; ++f) {
        a.n[f] = h->n[f];
        if ((host_mask >> f) & 1u) most += (int64_t)h->n[f] * fan;
    }
    const size_t room = (size_t)std::min<int64_t>(cap, most);   // entries the kernel may write
    if (room && !points) return fail(EDS_ERR_INVALID, "null points");
    if (room && on_device) {
        if ((rc = eds_dev_check_range(h->own.dev, points, room * 24))) return rc;
        if (colors && (rc = eds_dev_check_range(h->own.dev, colors, room * 32))) return rc;
        if (status && (rc = eds_dev_check_range(h->own.dev, status, room))) return rc;
    }
    if (!most) { *n_out = 0; return EDS_OK; }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t par_bytes = (size_t)n_hosts * 12 * sizeof(double), o_col = round16(room * 24), o_st = o_col + round16(room * 32);
    if ((rc = ensure_state(h->map, h->own, par_bytes + 2 * sizeof(int), on_device || !room ? 0 : o_st + round16(room)))) return rc;
    eds_map_state* s = h->map;
    std::memcpy(s->h_pin, T_w_c, par_bytes);
    int* h_n = reinterpret_cast<int*>(s->h_pin + par_bytes);
    h_n[0] = h_n[1] = 0;
    a.mask = host_mask; a.n_hosts = n_hosts; a.pitch = h->max_points; a.fan = fan; a.cap = (long long)cap;
    a.cal.fx = calib[0]; a.cal.fy = calib[1]; a.cal.cx = calib[2]; a.cal.cy = calib[3];
    double *d_pts = points, *d_col = colors;
    uint8_t* d_st = status;
    if (!on_device) {
        d_pts = reinterpret_cast<double*>(s->stage);
        d_col = colors ? reinterpret_cast<double*>(s->stage + o_col) : nullptr;
        d_st = status ? reinterpret_cast<uint8_t*>(s->stage + o_st) : nullptr;
    }
    hipLaunchKernelGGL(k_map_immature, dim3(1), dim3(CT), 0, h->own.st, a, h->points, reinterpret_cast<const double*>(s->d_pin),
                       reinterpret_cast<int*>(s->d_pin + par_bytes), d_pts, d_col, d_st);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<char> back;
    if (!on_device && room) {
        back.resize(o_st + round16(room));
        EDS_HIP_TRY(hipMemcpyAsync(back.data(), s->stage, back.size(), hipMemcpyDeviceToHost, h->own.st));
    }
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    *n_out = h_n[0];
    if (!h_n[1]) return fail(EDS_ERR_INVALID, "cap holds " + std::to_string(cap) + " entries, the cloud has " + std::to_string(h_n[0]));
    if (!on_device) {
        const size_t n = (size_t)h_n[0];
        if (n) std::memcpy(points, back.data(), n * 24);
        if (n && colors) std::memcpy(colors, back.data() + o_col, n * 32);
        if (n && status) std::memcpy(status, back.data() + o_st, n);
    }
    return EDS_OK;
}

int eds_map_set_immature_trace(eds_imm* h, int host, const float* idepth_min, const float* idepth_max, const int32_t* last_trace_status) {
    int rc;
    if ((rc = check_handle(h, "eds_imm"))) return rc;
    if (host < 0 || host >= h->max_hosts) return fail(EDS_ERR_INVALID, "host outside 0 .. max_hosts - 1");
    const int n = h->n[host];
    if (!n) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    std::vector<edsimm::Point> row((size_t)n);
    edsimm::Point* d_row = h->points + (size_t)host * h->max_points;
    if ((rc = read_back(h->own, row.data(), d_row, row.size() * sizeof(edsimm::Point)))) return rc;
    for (int i = 0; i < n; ++i) {
        if (idepth_min) row[i].idepth_min = idepth_min[i];
        if (idepth_max) row[i].idepth_max = idepth_max[i];
        if (last_trace_status) row[i].status = last_trace_status[i];
    }
    EDS_HIP_TRY(hipMemcpyAsync(d_row, row.data(), row.size() * sizeof(edsimm::Point), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_map_slot_cloud(eds_trk* h, int first, int count, const double* T_w_kf, int stride, double* points, int on_device, int* n_out) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (!T_w_kf || !points || !n_out) return fail(EDS_ERR_INVALID, "null T_w_kf, points or n_out");
    if (!edsmap::finite_all(T_w_kf, 12 * (int64_t)count)) return fail(EDS_ERR_INVALID, "T_w_kf is not finite");
    if ((rc = check_flag(on_device, "on_device"))) return rc;
    const int maxN = max_points(h, first, count);
    if (stride < maxN || stride < 1) return fail(EDS_ERR_INVALID, "stride smaller than the largest point count");
    if ((rc = check_idle_slots(h, first, count, EDS_NEED_KF))) return rc;
    const size_t extent = ((size_t)(count - 1) * (size_t)stride + (size_t)h->slots[first + count - 1].N) * 24;
    if (on_device && (rc = eds_dev_check_range(h->own.dev, points, extent))) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t Np = (size_t)h->Np;
    if (!on_device && (rc = ensure_state(h->map, h->own, 0, (size_t)SLOT_BATCH * Np * 24))) return rc;
    std::vector<double> back;
    for (int c0 = 0; c0 < count; c0 += SLOT_BATCH) {
        const int cn = std::min(SLOT_BATCH, count - c0);
        SlotArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int b = 0; b < cn; ++b) a.seeded[b] = h->slots[first + c0 + b].seeded ? 1 : 0;
        std::memcpy(a.T, T_w_kf + 12 * (size_t)c0, 12 * (size_t)cn * sizeof(double));
        double* dst = on_device ? points + (size_t)c0 * (size_t)stride * 3 : reinterpret_cast<double*>(h->map->stage);
        const long long st = on_device ? (long long)stride : (long long)Np;
        hipLaunchKernelGGL(k_map_slot_cloud, dim3(blocks(max_points(h, first + c0, cn), TB), cn), dim3(TB), 0, h->own.st, h->arrays(), a, first + c0,
                           h->depth.seeds, st, dst);
        EDS_HIP_TRY(hipGetLastError());
        if (!on_device) {
            back.resize((size_t)cn * Np * 3);
            EDS_HIP_TRY(hipMemcpyAsync(back.data(), dst, back.size() * sizeof(double), hipMemcpyDeviceToHost, h->own.st));
        }
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
        for (int b = 0; !on_device && b < cn; ++b)
            std::memcpy(points + (size_t)(c0 + b) * (size_t)stride * 3, back.data() + (size_t)b * Np * 3, (size_t)h->slots[first + c0 + b].N * 24);
    }
    for (int b = 0; b < count; ++b) n_out[b] = h->slots[first + b].N;
    return EDS_OK;
}

}  // extern "C"
