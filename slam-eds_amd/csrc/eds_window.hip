// include/eds_hip_window.h: the per-residual and per-point part of DSO's window optimiser on the device.  The arithmetic is
// eds_window.hpp, shared with the host; this file holds the kernels and the C entry points.  Built without contraction into FMAs
// (csrc/Makefile).
//
// k_win_linearize gives a residual EIGHT lanes, eight residuals per wavefront: the eight taps of the pattern are independent, so lane j
// fetches and evaluates tap j (edswin::tap, the host's code).  The geometric prologue runs on all eight lanes from the same values.
// Every lane then reads the octet's taps with width-8 shuffles and adds the twelve running sums in pattern order 0 ... 7, which is the
// serial rounding; the first failing tap in pattern order comes from a ballot over the octet.  The (host, target) records sit in LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_window.h"
#include "eds_capi_internal.hpp"
#include "eds_window.hpp"
#include "eds_window_internal.hpp"

using edscapi::blocks;
using edscapi::fail;
using edscapi::read_back;
using edswin::Calib;
using edswin::Params;
using edswin::Point;
using edswin::PointOut;
using edswin::Precalc;
using edswin::Px;
using edswin::J_WORDS;
using edswin::Sum;

static_assert(sizeof(Params) == sizeof(eds_win_params), "edswin::Params is eds_win_params member for member");
static_assert(sizeof(Precalc) == EDS_WIN_PRECALC_FLOATS * sizeof(float), "one precalc record is 27 floats");
static_assert(edswin::MAX_FRAMES == EDS_WIN_MAX_FRAMES && J_WORDS == EDS_WIN_J_WORDS, "header constants");
static_assert(sizeof(PointOut) == 10 * sizeof(float), "ten words per point");

namespace {

constexpr int TB = 256;

struct Dev {
    const int32_t *res_point, *res_target;
    int32_t *state, *new_state, *active;
    float *energy, *new_energy, *new_energy_wo, *ret, *cp, *proj, *J, *efJ, *JpJdF;
};

__device__ inline float pick8(int j, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    return j == 0 ? a0 : j == 1 ? a1 : j == 2 ? a2 : j == 3 ? a3 : j == 4 ? a4 : j == 5 ? a5 : j == 6 ? a6 : a7;
}

__global__ void __launch_bounds__(TB) k_win_linearize(Calib K, Params s, int F, const Precalc* __restrict__ pcs, const float* __restrict__ th,
                                                      const Px* __restrict__ frames, const Point* __restrict__ pts, const float* __restrict__ ids,
                                                      const float* __restrict__ idz, Dev t, int m, const int32_t* __restrict__ mask) {
    __shared__ float sh_pc[edswin::MAX_FRAMES * edswin::MAX_FRAMES * 27];
    for (int k = threadIdx.x; k < F * F * 27; k += TB) sh_pc[k] = reinterpret_cast<const float*>(pcs)[k];
    __syncthreads();
    const int gid = blockIdx.x * TB + threadIdx.x, j = gid & 7, lane = threadIdx.x & 63;
    const bool valid = (gid >> 3) < m;
    const int i = valid ? gid >> 3 : m - 1;                     // the spare octets of the last wavefront redo the last residual and store nothing
    const bool entry_oob = t.state[i] == edswin::ST_OOB;
    const int ip = t.res_point[i], tg = t.res_target[i];
    if (mask && !mask[ip]) return;                              // include/eds_hip_winflag.h: only the residuals of the points marked; a whole octet leaves
    const Point* pt = pts + ip;
    const int host = pt->host;
    Precalc pc;
    {
        const float* src = sh_pc + (host * F + tg) * 27;
        float* dst = reinterpret_cast<float*>(&pc);
#pragma unroll
        for (int k = 0; k < 27; ++k) dst[k] = src[k];
    }
    const edswin::Geo g = edswin::geo(K, s, pc, pt->u, pt->v, idz[ip]);
    const bool go = !entry_oob && g.ok;
    edswin::Tap o;
    o.fail = 0;
    o.Ku = o.Kv = o.resF = o.jx = o.jy = o.ja = o.jb = o.e = o.wji2 = 0.0f;
#pragma unroll
    for (int q = 0; q < 10; ++q) o.s[q] = 0.0f;
    if (go) o = edswin::tap(K, s, pc, frames + (size_t)tg * K.W * K.H, *pt, ids[ip], j);
    // the first failing tap in pattern order
    const unsigned long long bal = __ballot(go && o.fail != 0);
    const unsigned oct = (unsigned)(bal >> (lane & ~7)) & 0xffu;
    const int first = oct ? __ffs((int)oct) - 1 : 8;
    edswin::Sums a = edswin::sums_zero();
#pragma unroll
    for (int k = 0; k < edswin::PATTERN; ++k) {
        float sk[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) sk[q] = __shfl(o.s[q], k, 8);
        edswin::sums_add(a, __shfl(o.e, k, 8), __shfl(o.wji2, k, 8), sk);
    }
    if (!valid) return;
    const float old_energy = t.energy[i];
    if (go && (j < first || (j == first && o.fail == 2))) { t.proj[(size_t)i * 16 + 2 * j] = o.Ku; t.proj[(size_t)i * 16 + 2 * j + 1] = o.Kv; }
    if (go && j < 3) t.cp[(size_t)i * 3 + j] = j == 0 ? g.cp[0] : j == 1 ? g.cp[1] : g.cp[2];
    if (!go || first < 8) {
        if (j == 0) { t.new_energy_wo[i] = -1.0f; t.new_state[i] = edswin::ST_OOB; t.ret[i] = old_energy; }
        return;
    }
    float* J = t.J + (size_t)i * J_WORDS;
    J[edswin::J_RESF + j] = o.resF;
    J[edswin::J_JIDX + j] = o.jx; J[edswin::J_JIDX + 8 + j] = o.jy;
    J[edswin::J_JABF + j] = o.ja; J[edswin::J_JABF + 8 + j] = o.jb;
    // words 8 .. 29 (Jpdxi, Jpdc, Jpdd) and 62 .. 73 (JIdx2, JabJIdx, Jab2) are the same in the eight lanes: lane j stores every eighth
    J[8 + j] = pick8(j, g.Jpdxi[0], g.Jpdxi[1], g.Jpdxi[2], g.Jpdxi[3], g.Jpdxi[4], g.Jpdxi[5], g.Jpdxi[6], g.Jpdxi[7]);
    J[16 + j] = pick8(j, g.Jpdxi[8], g.Jpdxi[9], g.Jpdxi[10], g.Jpdxi[11], g.Jpdc[0], g.Jpdc[1], g.Jpdc[2], g.Jpdc[3]);
    if (j < 6) J[24 + j] = pick8(j, g.Jpdc[4], g.Jpdc[5], g.Jpdc[6], g.Jpdc[7], g.Jpdd[0], g.Jpdd[1], 0.0f, 0.0f);
    J[62 + j] = pick8(j, a.s[0], a.s[2], a.s[2], a.s[1], a.s[3], a.s[4], a.s[5], a.s[6]);
    if (j < 4) J[70 + j] = pick8(j, a.s[7], a.s[8], a.s[8], a.s[9], 0.0f, 0.0f, 0.0f, 0.0f);
    if (j == 0) {
        const edswin::Verdict v = edswin::verdict(a, th[host], th[tg]);
        t.new_energy_wo[i] = v.energy_with_outlier;
        t.new_state[i] = v.state;
        t.new_energy[i] = v.energy;
        t.ret[i] = v.energy;
    }
}

using edsdso::wave_fold;                                        // the fold inside 64 lanes is eds_dso_common.hpp's, as is add8
using edsdso::wave_fold_i;

// the energy in the header's sum order and the counts of the new states, one workgroup
__global__ void __launch_bounds__(edswin::LANES) k_win_energy(const float* __restrict__ ret, const int32_t* __restrict__ new_state, int m, Sum* out) {
    __shared__ double part[8];
    __shared__ int ipart[24];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double e = 0.0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int i = threadIdx.x; i < m; i += 8 * edswin::LANES) {   // eight loads in flight per trip; the adds keep the lane's order
        float r[8];
        int st[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = i + k * edswin::LANES, qc = q < m ? q : m - 1;        // unconditional loads: the eight stay in flight together
            r[k] = ret[qc];
            st[k] = q < m ? new_state[qc] : -1;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (st[k] >= 0) e += (double)r[k];
            c0 += st[k] == 0; c1 += st[k] == 1; c2 += st[k] == 2;
        }
    }
    e = wave_fold(e); c0 = wave_fold_i(c0); c1 = wave_fold_i(c1); c2 = wave_fold_i(c2);
    if (lane == 0) { part[wave] = e; ipart[wave] = c0; ipart[8 + wave] = c1; ipart[16 + wave] = c2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out->energy = edsdso::add8(part);
        for (int k = 0; k < 3; ++k) {
            int c = 0;
            for (int w = 0; w < 8; ++w) c += ipart[8 * k + w];
            out->counts[k] = c;
        }
        out->counts[3] = 0;
    }
}

// applyRes for one residual per octet of lanes: lane j copies every eighth word of J (edswin::apply_one's copy, coalesced), lane 0 forms
// JpJdF from the words it copied from and moves the state
__global__ void __launch_bounds__(TB) k_win_apply(Dev t, int m, int copy_jacobians, const int32_t* __restrict__ mask) {
    const int gid = blockIdx.x * TB + threadIdx.x, i = gid >> 3, j = gid & 7;
    if (i >= m || (mask && !mask[t.res_point[i]])) return;
    // All eight lanes read the state before lane 0 stores it below.  That is ordered: an octet lies inside ONE wavefront (8 divides 64
    // and TB), a wavefront runs its instructions in program order for all its lanes, and these loads come before the store.
    const int st = t.state[i], ns = t.new_state[i];
    if (copy_jacobians) {
        if (st == edswin::ST_OOB) return;
        if (ns == edswin::ST_IN) {
            const float* src = t.J + (size_t)i * J_WORDS;
            float* dst = t.efJ + (size_t)i * J_WORDS;
            for (int k = j; k < J_WORDS; k += 8) dst[k] = src[k];
            if (j == 0) { t.active[i] = 1; edswin::jpjdf(src, t.JpJdF + (size_t)i * 8); }
        } else if (j == 0) {
            t.active[i] = 0;
        }
    }
    if (j == 0) { t.state[i] = ns; t.energy[i] = t.new_energy[i]; }
}

// addPoint<0>'s per-point sums (mode 2: zero, for the points of sel) and the Schur complement's per-point prologue, one thread per point;
// nres, the residuals added, is an integer atomic
__global__ void __launch_bounds__(TB) k_win_points(int n, const int32_t* __restrict__ res_first, const int32_t* __restrict__ active,
                                                   const int32_t* __restrict__ lin, int mode, const int32_t* __restrict__ sel,
                                                   const float* __restrict__ efJ, const float* __restrict__ prior, const float* __restrict__ delta,
                                                   const float* __restrict__ lf, int has_prior, int has_delta, int has_lf, int shift,
                                                   PointOut* __restrict__ out, int32_t* nres) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= n || (sel && !sel[p])) return;
    float l[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (has_lf) {
#pragma unroll
        for (int k = 0; k < 6; ++k) l[k] = lf[6 * p + k];
    }
    int added = 0;
    const PointOut o = edswin::point_sums_mode(active, lin, efJ, res_first[p], res_first[p + 1], has_prior ? prior[p] : 0.0f,
                                               has_delta ? delta[p] : 0.0f, l, shift != 0, mode, &added);
    out[p] = o;
    if (added) atomicAdd(nres, added);
}

// one accumulator word per workgroup: the 512 lanes stride the host frame's points, fold as the header says
__global__ void __launch_bounds__(edswin::LANES) k_win_acc(edswin::AccIn in, double* __restrict__ acc) {
    __shared__ double part[8];
    const int j = blockIdx.x, h = edswin::acc_host(in.F, j), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = in.first[h], p1 = in.first[h + 1];
    double v = 0.0;
    for (int p = p0 + (int)threadIdx.x; p < p1; p += edswin::LANES) v += edswin::acc_value(in, j, p);
    v = wave_fold(v);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) acc[j] = edsdso::add8(part);
}

// both stitches, one thread per output entry (edswin::stitch_entry: the addends and their order are stitch_serial's)
__global__ void __launch_bounds__(TB) k_win_stitch(int F, const double* __restrict__ acc, const double* __restrict__ adH, const double* __restrict__ adT,
                                                   int entries, double* __restrict__ out) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e < entries) edswin::stitch_entry(F, acc, adH, adT, e, out);
}

Dev tables(const eds_win* h) {
    Dev t = {h->res_point, h->res_target, h->state, h->new_state, h->active, h->energy, h->new_energy, h->new_energy_wo, h->ret, h->cp, h->proj,
             h->J, h->efJ, h->JpJdF};
    return t;
}
bool all_finite_f(const float* x, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false;
    return true;
}
// the (point, target) -> residual map and the hosts' runs [first[h], first[h + 1])
int build_maps(const eds_win* h, int F, std::vector<int32_t>& res_of, std::vector<int32_t>& first) {
    res_of.assign((size_t)h->n * F, -1);
    first.assign((size_t)9, h->n);
    for (int i = 0; i < h->m; ++i) {
        int32_t& slot = res_of[(size_t)h->h_point[i] * F + h->h_target[i]];
        if (slot >= 0) return fail(EDS_ERR_INVALID, "a point has two residuals towards one target");
        slot = i;
    }
    // the fold walks [first[h], first[h + 1]): the hosts' runs must tile 0 .. n in host order
    for (int p = 1; p < h->n; ++p)
        if (h->host_of[p] < h->host_of[p - 1]) return fail(EDS_ERR_INVALID, "eds_win_accumulate needs the points in nondecreasing host order");
    for (int f = 0, p = 0; f < 9; ++f) {
        first[f] = p;
        while (p < h->n && h->host_of[p] == f) ++p;
    }
    return EDS_OK;
}
template <class T> int download(eds_win* h, T* dst, const T* src, size_t n) { return read_back(h->own, dst, src, n * sizeof(T)); }

}  // namespace

namespace edswin_internal {

int upload_maps(eds_win* h, int F) {
    std::vector<int32_t> res_of, first;
    if (int rc = build_maps(h, F, res_of, first)) return rc;
    if (h->n) EDS_HIP_TRY(hipMemcpyAsync(h->res_of, res_of.data(), res_of.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->first, first.data(), 9 * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));                  // the two vectors end here
    return EDS_OK;
}

void queue_points(eds_win* h, int mode, const int32_t* sel, int shift) {
    if (!h->n) return;
    (void)hipMemsetAsync(h->nres, 0, sizeof(int32_t), h->own.st);
    hipLaunchKernelGGL(k_win_points, dim3(blocks((size_t)h->n)), dim3(TB), 0, h->own.st, h->n, h->res_first, h->active, lin_flags(h), mode, sel, h->efJ,
                       h->prior, h->delta, h->lf, 1, 1, lf_on_device(h) ? 1 : 0, shift, h->pout, h->nres);
}

void queue_acc(eds_win* h, int F, int mode, const int32_t* sel, int has_lf, int words, double* acc) {
    const edswin::AccIn in = {F, has_lf, h->first, h->res_of, h->active, h->efJ, h->JpJdF, h->pout, h->lf,
                              mode, lin_flags(h), h->wsv ? h->wsv->res_approx : nullptr, sel};
    hipLaunchKernelGGL(k_win_acc, dim3((unsigned)words), dim3(edswin::LANES), 0, h->own.st, in, acc);
}

void queue_apply(eds_win* h, int copy_jacobians, const int32_t* mask) {
    if (!h->m) return;
    hipLaunchKernelGGL(k_win_apply, dim3(blocks((size_t)h->m * 8)), dim3(TB), 0, h->own.st, tables(h), h->m, copy_jacobians, mask);
}
void queue_linearize(eds_win* h, int F, const int32_t* mask) {
    if (!h->m) return;
    hipLaunchKernelGGL(k_win_linearize, dim3(blocks((size_t)h->m * 8)), dim3(TB), 0, h->own.st, h->cal, h->prm, F, h->pcs, h->th, h->frames, h->pts, h->ids, h->idz,
                       tables(h), h->m, mask);
}

void queue_stitch(eds_win* h, int F, const double* acc, const double* ad, int entries, double* out) {
    hipLaunchKernelGGL(k_win_stitch, dim3(blocks((size_t)entries)), dim3(TB), 0, h->own.st, F, acc, ad, ad + (size_t)F * F * 64, entries, out);
}

}  // namespace edswin_internal

extern "C" {

int eds_win_abi_version(void) { return EDS_HIP_WINDOW_ABI_VERSION; }

void eds_win_params_default(eds_win_params* p) {
    if (!p) return;
    const Params d = edswin::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_win_create(int device, int H, int W, int max_frames, int max_points, int max_residuals, eds_win** win) {
    if (!win) return fail(EDS_ERR_INVALID, "null output");
    *win = nullptr;
    if (!edswin::shape_valid(H, W)) return fail(EDS_ERR_INVALID, "H and W are 8 .. 8192");
    if (max_frames < 2 || max_frames > EDS_WIN_MAX_FRAMES) return fail(EDS_ERR_INVALID, "max_frames is 2 .. 8");
    if (max_points < 1 || max_points > (1 << 22) || max_residuals < 1 || max_residuals > (1 << 24))
        return fail(EDS_ERR_INVALID, "max_points is 1 .. 2^22, max_residuals 1 .. 2^24");
    eds_win* h = new eds_win;
    if (int rc = h->own.open(device)) { delete h; return rc; }
    h->H = H; h->W = W; h->max_frames = max_frames; h->max_points = max_points; h->max_residuals = max_residuals;
    h->prm = edswin::params_default();
    const size_t px = (size_t)H * W, mp = (size_t)max_points, mr = (size_t)max_residuals;
    const bool ok = h->own.alloc({{(void**)&h->frames, px * max_frames * sizeof(Px)},
                                  {(void**)&h->in_img, px * sizeof(float)},
                                  {(void**)&h->pts, mp * sizeof(Point)},
                                  {(void**)&h->ids, mp * sizeof(float)},
                                  {(void**)&h->idz, mp * sizeof(float)},
                                  {(void**)&h->res_first, (mp + 1) * sizeof(int32_t)},
                                  {(void**)&h->res_point, mr * sizeof(int32_t)},
                                  {(void**)&h->res_target, mr * sizeof(int32_t)},
                                  {(void**)&h->state, mr * sizeof(int32_t)},
                                  {(void**)&h->new_state, mr * sizeof(int32_t)},
                                  {(void**)&h->active, mr * sizeof(int32_t)},
                                  {(void**)&h->energy, mr * sizeof(float)},
                                  {(void**)&h->new_energy, mr * sizeof(float)},
                                  {(void**)&h->new_energy_wo, mr * sizeof(float)},
                                  {(void**)&h->ret, mr * sizeof(float)},
                                  {(void**)&h->cp, mr * 3 * sizeof(float)},
                                  {(void**)&h->proj, mr * 16 * sizeof(float)},
                                  {(void**)&h->J, mr * J_WORDS * sizeof(float)},
                                  {(void**)&h->efJ, mr * J_WORDS * sizeof(float)},
                                  {(void**)&h->JpJdF, mr * 8 * sizeof(float)},
                                  {(void**)&h->th, 8 * sizeof(float)},
                                  {(void**)&h->prior, mp * sizeof(float)},
                                  {(void**)&h->delta, mp * sizeof(float)},
                                  {(void**)&h->lf, mp * 6 * sizeof(float)},
                                  {(void**)&h->pcs, 64 * sizeof(Precalc)},
                                  {(void**)&h->sum, sizeof(Sum)},
                                  {(void**)&h->pout, mp * sizeof(PointOut)},
                                  {(void**)&h->nres, sizeof(int32_t)},
                                  {(void**)&h->res_of, mp * 8 * sizeof(int32_t)},
                                  {(void**)&h->first, 9 * sizeof(int32_t)},
                                  {(void**)&h->acc, (size_t)edswin::acc_size(8) * sizeof(double)},
                                  {(void**)&h->ad, 2 * 64 * 64 * sizeof(double)},
                                  {(void**)&h->stitched, (size_t)edswin::stitch_words(8) * sizeof(double)}});
    if (!ok || hipMemsetAsync(h->pout, 0, mp * sizeof(PointOut), h->own.st) != hipSuccess ||
        hipMemsetAsync(h->res_first, 0, (mp + 1) * sizeof(int32_t), h->own.st) != hipSuccess || hipMemsetAsync(h->active, 0, mr * sizeof(int32_t), h->own.st) != hipSuccess ||
        hipStreamSynchronize(h->own.st) != hipSuccess) {
        (void)hipGetLastError();
        eds_win_destroy(h);
        return fail(EDS_ERR_HIP, "eds_win_create: the device refused a stream or an allocation");
    }
    *win = h;
    return EDS_OK;
}

void eds_win_destroy(eds_win* h) {
    if (!h) return;
    h->own.close();                                            // the window's buffers and both states', whichever set holds them now
    edswin_internal::wsv_release(h);
    edswin_internal::wed_release(h);
    edswin_internal::wfl_release(h);
    edsmap_internal::release(h->map);
    delete h;
}

int eds_win_set_params(eds_win* h, const eds_win_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null parameters");
    Params s;
    std::memcpy(&s, p, sizeof(s));
    if (!edswin::params_valid(s))
        return fail(EDS_ERR_INVALID, "parameters: every float finite; outlier_th_sum_component, huber_th and the scales > 0");
    h->prm = s;
    return EDS_OK;
}

int eds_win_get_params(const eds_win* h, eds_win_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(p, &h->prm, sizeof(*p));
    return EDS_OK;
}

int eds_win_set_calib(eds_win* h, float fx, float fy, float cx, float cy) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!edscapi::check_calib(fx, fy, cx, cy)) return fail(EDS_ERR_INVALID, "calibration: fx, fy, cx, cy finite, fx and fy > 0");
    h->cal = edswin::make_calib(h->H, h->W, fx, fy, cx, cy);
    h->calib_set = true;
    return EDS_OK;
}

int eds_win_set_frames(eds_win* h, int first, int count, const float* images, int64_t row_stride, int64_t frame_stride, int on_device) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    const int H = h->H, W = h->W;
    if (first < 0 || count < 1 || first > h->max_frames - count) return fail(EDS_ERR_INVALID, "frames first .. first + count - 1 outside the handle's");
    if (int rc = edscapi::check_images(h->own.dev, H, W, count, images, &row_stride, &frame_stride, on_device, "images")) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t px = (size_t)H * W;
    for (int f = 0; f < count; ++f) {
        h->frames_set &= ~(1u << (first + f));
        Px* dst = h->frames + (size_t)(first + f) * px;
        if (int rc = edscapi::upload_image(h->own, h->in_img, H, W, images + (int64_t)f * frame_stride, row_stride, on_device)) return rc;
        edscapi::queue_level(h->own.st, h->in_img, nullptr, 0, dst, W, H);
        EDS_HIP_TRY(hipGetLastError());
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));                // the host image may be pageable, and in_img is reused by the next frame
        h->frames_set |= 1u << (first + f);
    }
    return EDS_OK;
}

int eds_win_get_frame(eds_win* h, int frame, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (frame < 0 || frame >= h->max_frames) return fail(EDS_ERR_INVALID, "frame outside the handle's");
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!(h->frames_set >> frame & 1u)) return fail(EDS_ERR_STATE, "eds_win: that frame was never set");
    const size_t px = (size_t)h->H * h->W;
    std::vector<Px> p(px);
    if (int rc = read_back(h->own, p.data(), h->frames + (size_t)frame * px, px * sizeof(Px))) return rc;
    for (size_t i = 0; i < px; ++i) { out[3 * i] = p[i].c; out[3 * i + 1] = p[i].dx; out[3 * i + 2] = p[i].dy; }
    return EDS_OK;
}

int eds_win_set_points(eds_win* h, int n, const int32_t* host, const float* uv, const float* color, const float* weights,
                       const float* idepth_scaled, const float* idepth_zero_scaled) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (n < 0 || n > h->max_points) return fail(EDS_ERR_INVALID, std::to_string(n) + " points, the handle holds 0 .. " + std::to_string(h->max_points));
    if (n > 0 && (!host || !uv || !color || !weights || !idepth_scaled || !idepth_zero_scaled))
        return fail(EDS_ERR_INVALID, "host, uv, color, weights, idepth_scaled and idepth_zero_scaled are required");
    uint32_t closed = 0;                                        // hosts whose run has ended
    int max_host = -1;
    for (int i = 0; i < n; ++i) {
        if (host[i] < 0 || host[i] >= h->max_frames) return fail(EDS_ERR_INVALID, "point " + std::to_string(i) + ": host frame outside the handle's");
        if (i > 0 && host[i] != host[i - 1]) closed |= 1u << host[i - 1];
        if (closed >> host[i] & 1u) return fail(EDS_ERR_INVALID, "points must be grouped by host frame");
        if (host[i] > max_host) max_host = host[i];
    }
    std::vector<Point> p((size_t)n);
    for (int i = 0; i < n; ++i) {
        p[i].host = host[i]; p[i].u = uv[2 * i]; p[i].v = uv[2 * i + 1];
        for (int k = 0; k < 8; ++k) { p[i].color[k] = color[8 * i + k]; p[i].weights[k] = weights[8 * i + k]; }
    }
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (n) {
        EDS_HIP_TRY(hipMemcpyAsync(h->pts, p.data(), p.size() * sizeof(Point), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->ids, idepth_scaled, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->idz, idepth_zero_scaled, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    }
    // the residual table becomes empty ON THE DEVICE too: every point's run is [0, 0) and nothing is active
    EDS_HIP_TRY(hipMemsetAsync(h->res_first, 0, ((size_t)h->max_points + 1) * sizeof(int32_t), h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->active, 0, (size_t)h->max_residuals * sizeof(int32_t), h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->pout, 0, (size_t)h->max_points * sizeof(PointOut), h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->n = n; h->m = 0; h->max_host = max_host; h->max_target = -1; h->linearized = false;
    edswin_internal::wsv_invalidate(h);
    h->host_of.assign(host, host + n);
    h->h_point.clear(); h->h_target.clear();
    return h->wfl ? edswin_internal::wfl_reset(h) : (int)EDS_OK;
}

int eds_win_set_idepths(eds_win* h, const float* idepth_scaled, const float* idepth_zero_scaled) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!idepth_scaled && !idepth_zero_scaled) return fail(EDS_ERR_INVALID, "idepth_scaled or idepth_zero_scaled is required");
    if (!h->n) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t bytes = (size_t)h->n * sizeof(float);
    if (idepth_scaled) EDS_HIP_TRY(hipMemcpyAsync(h->ids, idepth_scaled, bytes, hipMemcpyHostToDevice, h->own.st));
    if (idepth_zero_scaled) EDS_HIP_TRY(hipMemcpyAsync(h->idz, idepth_zero_scaled, bytes, hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_win_set_residuals(eds_win* h, int m, const int32_t* point, const int32_t* target, const int32_t* state, const float* energy) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (m < 0 || m > h->max_residuals) return fail(EDS_ERR_INVALID, std::to_string(m) + " residuals, the handle holds 0 .. " + std::to_string(h->max_residuals));
    if (m > 0 && (!point || !target)) return fail(EDS_ERR_INVALID, "point and target are required");
    int max_target = -1;
    for (int i = 0; i < m; ++i) {
        if (point[i] < 0 || point[i] >= h->n) return fail(EDS_ERR_INVALID, "residual " + std::to_string(i) + ": no such point");
        if (i > 0 && point[i] < point[i - 1]) return fail(EDS_ERR_INVALID, "residuals must be grouped by point in nondecreasing point index");
        if (target[i] < 0 || target[i] >= h->max_frames) return fail(EDS_ERR_INVALID, "residual " + std::to_string(i) + ": target frame outside the handle's");
        if (target[i] == h->host_of[point[i]]) return fail(EDS_ERR_INVALID, "residual " + std::to_string(i) + ": its target is its host");
        if (state && (state[i] < 0 || state[i] > 2)) return fail(EDS_ERR_INVALID, "residual " + std::to_string(i) + ": state is 0 IN, 1 OOB or 2 OUTLIER");
        if (target[i] > max_target) max_target = target[i];
    }
    std::vector<int32_t> first((size_t)h->n + 1, 0), st((size_t)m, 0), ns((size_t)m, edswin::ST_OUTLIER);
    for (int i = 0; i < m; ++i) ++first[point[i] + 1];
    for (int p = 0; p < h->n; ++p) first[p + 1] += first[p];
    if (state) st.assign(state, state + m);
    std::vector<float> en((size_t)m, 0.0f);
    if (energy) en.assign(energy, energy + m);
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t mm = (size_t)m;
    EDS_HIP_TRY(hipMemcpyAsync(h->res_first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    if (m) {
        EDS_HIP_TRY(hipMemcpyAsync(h->res_point, point, mm * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->res_target, target, mm * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->state, st.data(), mm * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->new_state, ns.data(), mm * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->energy, en.data(), mm * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->new_energy, en.data(), mm * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->active, 0, mm * sizeof(int32_t), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->new_energy_wo, 0, mm * sizeof(float), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->ret, 0, mm * sizeof(float), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->cp, 0, mm * 3 * sizeof(float), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->proj, 0, mm * 16 * sizeof(float), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->J, 0, mm * J_WORDS * sizeof(float), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->efJ, 0, mm * J_WORDS * sizeof(float), h->own.st));
        EDS_HIP_TRY(hipMemsetAsync(h->JpJdF, 0, mm * 8 * sizeof(float), h->own.st));
    }
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->m = m; h->max_target = max_target; h->linearized = false;
    edswin_internal::wsv_invalidate(h);
    h->h_point.assign(point, point + m); h->h_target.assign(target, target + m);
    return h->wfl ? edswin_internal::wfl_reset(h) : (int)EDS_OK;
}

int eds_win_linearize(eds_win* h, int F, const float* precalc, const float* frame_energy_th, double* energy, int32_t* counts) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (F < 2 || F > h->max_frames) return fail(EDS_ERR_INVALID, "F is 2 .. max_frames");
    if (!precalc || !frame_energy_th) return fail(EDS_ERR_INVALID, "precalc and frame_energy_th are required");
    if (!h->calib_set) return fail(EDS_ERR_STATE, "eds_win: no calibration set");
    if (h->max_host >= F || h->max_target >= F) return fail(EDS_ERR_INVALID, "a point's host or a residual's target is not below F");
    for (int f = 0; f < F; ++f)
        if (!(h->frames_set >> f & 1u)) return fail(EDS_ERR_STATE, "eds_win: frame " + std::to_string(f) + " was never set");
    if (!all_finite_f(precalc, (size_t)F * F * 27)) return fail(EDS_ERR_INVALID, "precalc is not finite");
    if (!all_finite_f(frame_energy_th, (size_t)F)) return fail(EDS_ERR_INVALID, "frame_energy_th is not finite");
    Sum back;
    back.energy = 0.0; back.counts[0] = back.counts[1] = back.counts[2] = back.counts[3] = 0;
    if (h->m) {
        EDS_HIP_TRY(hipSetDevice(h->own.dev));
        EDS_HIP_TRY(hipMemcpyAsync(h->pcs, precalc, (size_t)F * F * sizeof(Precalc), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(h->th, frame_energy_th, (size_t)F * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        edswin_internal::queue_linearize(h, F, nullptr);
        hipLaunchKernelGGL(k_win_energy, dim3(1), dim3(edswin::LANES), 0, h->own.st, h->ret, h->new_state, h->m, h->sum);
        EDS_HIP_TRY(hipGetLastError());
        if (int rc = read_back(h->own, &back, h->sum, sizeof(back))) return rc;
    }
    h->linearized = true;
    if (energy) *energy = back.energy;
    if (counts) for (int k = 0; k < 3; ++k) counts[k] = back.counts[k];
    return EDS_OK;
}

int eds_win_apply(eds_win* h, int copy_jacobians) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (copy_jacobians != 0 && copy_jacobians != 1) return fail(EDS_ERR_INVALID, "copy_jacobians is 0 or 1");
    if (!h->linearized) return fail(EDS_ERR_STATE, "eds_win_apply before eds_win_linearize");
    if (!h->m) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    edswin_internal::queue_apply(h, copy_jacobians, nullptr);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int eds_win_point_hessians(eds_win* h, const float* priorF, const float* deltaF, const float* lf, int shift_prior_to_zero, int32_t* nres) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (shift_prior_to_zero != 0 && shift_prior_to_zero != 1) return fail(EDS_ERR_INVALID, "shift_prior_to_zero is 0 or 1");
    const size_t n = (size_t)h->n;
    if ((priorF && !all_finite_f(priorF, n)) || (deltaF && !all_finite_f(deltaF, n)) || (lf && !all_finite_f(lf, 6 * n)))
        return fail(EDS_ERR_INVALID, "priorF, deltaF or the linearized sums are not finite");
    int32_t back = 0;
    if (n) {
        EDS_HIP_TRY(hipSetDevice(h->own.dev));
        if (priorF) EDS_HIP_TRY(hipMemcpyAsync(h->prior, priorF, n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        if (deltaF) EDS_HIP_TRY(hipMemcpyAsync(h->delta, deltaF, n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
        if (lf) {
            EDS_HIP_TRY(hipMemcpyAsync(h->lf, lf, 6 * n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
            if (h->wsv) h->wsv->lf_on_device = false;           // the caller's sums replace what modes 1 / 2 left there
        }
        EDS_HIP_TRY(hipMemsetAsync(h->nres, 0, sizeof(int32_t), h->own.st));
        // lf == NULL: the sums modes 1 / 2 of include/eds_hip_winsolve.h left on the device, when there are any
        hipLaunchKernelGGL(k_win_points, dim3(blocks(n)), dim3(TB), 0, h->own.st, h->n, h->res_first, h->active, edswin_internal::lin_flags(h), 0,
                           (const int32_t*)nullptr, h->efJ, h->prior, h->delta, h->lf, priorF ? 1 : 0, deltaF ? 1 : 0,
                           lf || edswin_internal::lf_on_device(h) ? 1 : 0, shift_prior_to_zero, h->pout, h->nres);
        EDS_HIP_TRY(hipGetLastError());
        if (int rc = read_back(h->own, &back, h->nres, sizeof(back))) return rc;
    }
    if (nres) *nres = back;
    return EDS_OK;
}

int eds_win_accumulate(eds_win* h, int F, const double* adHost, const double* adTarget, const float* priorF, const float* deltaF, const float* lf,
                       int shift_prior_to_zero, double* H_A, double* b_A, double* H_sc, double* b_sc, double* acc_out, int32_t* nres) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (F < 2 || F > h->max_frames) return fail(EDS_ERR_INVALID, "F is 2 .. max_frames");
    if (!adHost || !adTarget) return fail(EDS_ERR_INVALID, "adHost and adTarget are required");
    if (h->max_host >= F || h->max_target >= F) return fail(EDS_ERR_INVALID, "a point's host or a residual's target is not below F");
    for (size_t i = 0; i < (size_t)F * F * 64; ++i)
        if (!std::isfinite(adHost[i]) || !std::isfinite(adTarget[i])) return fail(EDS_ERR_INVALID, "the adjoints are not finite");
    std::vector<int32_t> res_of, first;
    if (int rc = build_maps(h, F, res_of, first)) return rc;
    if (int rc = eds_win_point_hessians(h, priorF, deltaF, lf, shift_prior_to_zero, nres)) return rc;
    const int words = edswin::acc_size(F);
    std::vector<double> acc((size_t)words, 0.0);
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (h->n) EDS_HIP_TRY(hipMemcpyAsync(h->res_of, res_of.data(), res_of.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->first, first.data(), 9 * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    edswin_internal::queue_acc(h, F, 0, nullptr, lf || edswin_internal::lf_on_device(h) ? 1 : 0, words, h->acc);
    EDS_HIP_TRY(hipGetLastError());
    const size_t N = 4 + 8 * (size_t)F, ad_words = (size_t)F * F * 64;
    const int sw = edswin::stitch_words(F);
    EDS_HIP_TRY(hipMemcpyAsync(h->ad, adHost, ad_words * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->ad + ad_words, adTarget, ad_words * sizeof(double), hipMemcpyHostToDevice, h->own.st));
    edswin_internal::queue_stitch(h, F, h->acc, h->ad, sw, h->stitched);
    EDS_HIP_TRY(hipGetLastError());
    std::vector<double> st((size_t)sw);
    EDS_HIP_TRY(hipMemcpyAsync(st.data(), h->stitched, st.size() * sizeof(double), hipMemcpyDeviceToHost, h->own.st));
    if (acc_out) EDS_HIP_TRY(hipMemcpyAsync(acc.data(), h->acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, h->own.st));   // only when asked for
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    if (H_A) std::memcpy(H_A, st.data(), N * N * sizeof(double));
    if (b_A) std::memcpy(b_A, st.data() + N * N, N * sizeof(double));
    if (H_sc) std::memcpy(H_sc, st.data() + N * N + N, N * N * sizeof(double));
    if (b_sc) std::memcpy(b_sc, st.data() + 2 * N * N + N, N * sizeof(double));
    if (acc_out) std::memcpy(acc_out, acc.data(), acc.size() * sizeof(double));
    return EDS_OK;
}

int eds_win_get_residuals(eds_win* h, const eds_win_residual_out* out) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    const size_t m = (size_t)h->m;
    if (!m) return EDS_OK;
    if (int rc = download(h, out->state, h->state, m)) return rc;
    if (int rc = download(h, out->energy, h->energy, m)) return rc;
    if (int rc = download(h, out->new_state, h->new_state, m)) return rc;
    if (int rc = download(h, out->new_energy, h->new_energy, m)) return rc;
    if (int rc = download(h, out->new_energy_with_outlier, h->new_energy_wo, m)) return rc;
    if (int rc = download(h, out->linearize_return, h->ret, m)) return rc;
    if (int rc = download(h, out->is_active, h->active, m)) return rc;
    if (int rc = download(h, out->center_projected_to, h->cp, 3 * m)) return rc;
    if (int rc = download(h, out->projected_to, h->proj, 16 * m)) return rc;
    if (int rc = download(h, out->J, h->J, J_WORDS * m)) return rc;
    if (int rc = download(h, out->ef_J, h->efJ, J_WORDS * m)) return rc;
    return download(h, out->JpJdF, h->JpJdF, 8 * m);
}

int eds_win_acc_size(int F) { return F >= 2 && F <= EDS_WIN_MAX_FRAMES ? edswin::acc_size(F) : 0; }

int eds_win_get_points(eds_win* h, const eds_win_point_out* out) {
    if (int rc = edscapi::check_handle(h, "eds_win")) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    const size_t n = (size_t)h->n;
    if (!n) return EDS_OK;
    std::vector<PointOut> p(n);
    if (int rc = read_back(h->own, p.data(), h->pout, n * sizeof(PointOut))) return rc;
    for (size_t i = 0; i < n; ++i) {
        if (out->Hdd_accAF) out->Hdd_accAF[i] = p[i].Hdd_accAF;
        if (out->bd_accAF) out->bd_accAF[i] = p[i].bd_accAF;
        if (out->Hcd_accAF) std::memcpy(out->Hcd_accAF + 4 * i, p[i].Hcd_accAF, 4 * sizeof(float));
        if (out->HdiF) out->HdiF[i] = p[i].HdiF;
        if (out->bdSumF) out->bdSumF[i] = p[i].bdSumF;
        if (out->idepth_hessian) out->idepth_hessian[i] = p[i].idepth_hessian;
        if (out->nres) out->nres[i] = p[i].nres;
    }
    return EDS_OK;
}

}  // extern "C"
