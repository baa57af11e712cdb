// include/eds_hip_select.h: DSO's pixel selector on the device.  Every piece of arithmetic and every decision is eds_pixsel.hpp, shared
// with the host; this file holds the kernels and the C entry points.  Built without contraction into FMAs (csrc/Makefile).
//
// One select pass is three kernels around the only serial dependence of the reference's loop, the running count n2 that picks every
// cell's direction (eds_pixsel.hpp, THE n2 CHAIN):
//   k_sel_hits   one thread per pot cell, in visiting order: the 16-bit mask of the directions under which the cell selects.
//   k_sel_scan   one workgroup walks the cells 1 024 at a time: an exclusive prefix sum over the certain cells (mask 0x0000 or 0xFFFF)
//                and over the ambiguous ones, then one lane resolves the chunk's ambiguous cells in order against the table; a chunk
//                without ambiguous cells — every chunk of an ordinary image — is the two scans alone.
//   k_sel_pick   one wavefront-sized workgroup per 4 pot block, looping over its pixels for any potential: the arg-max at the three
//                levels on the key (dirNorm, visiting order) with 64-bit integer atomics in LDS, then the block's up to 21 writes.
// k_sel_hist is one workgroup per 32 x 32 block with the histogram in LDS and the quantile in the same kernel; the sub-selection and
// the selection list are the stable compaction of eds_coarse.hip (k_ct_select): per-256 counts, then ranks from the counts before.
// The decisions of makeMaps between passes are edspix::decide on the host, from three integers read back per pass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_select.h"
#include "eds_capi_internal.hpp"
#include "eds_pixsel.hpp"
#include "eds_pixsel_internal.hpp"

using edscapi::blocks;
using edscapi::fail;
using edscapi::read_back;
using edspix::Block;
using edspix::Geo;
using edspix::Key;
using edspix::Params;
using edspix::Px;
using edspix::Sel;
using edspix::SLOTS;

static_assert(sizeof(Params) == sizeof(eds_sel_params), "edspix::Params is eds_sel_params member for member");
static_assert(sizeof(edspix::Pass) == sizeof(eds_sel_pass), "edspix::Pass is eds_sel_pass member for member");
static_assert(sizeof(Px) == 4 * sizeof(float), "a level reads back as {colour, dx, dy, absSquaredGrad}");
static_assert(edspix::MAX_POTENTIAL == EDS_SEL_MAX_POTENTIAL, "header constant");

namespace {

constexpr int TB = 256;
constexpr int SCAN = 1024;
constexpr int PICK = 64;
enum { C_N2 = 0, C_N3 = 1, C_N4 = 2, C_AMBIGUOUS = 3, C_N2_CERTAIN = 4, C_LIST = 5, C_COUNTS = 8 };

__global__ void __launch_bounds__(TB) k_sel_gradient(Px* p, int w, int h, const float* __restrict__ B) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= w * h) return;
    edspix::gradient_pixel(p, w, h, i, B);
}

// one workgroup per 32 x 32 block: hist[0] the pixels counted, hist[1 + g] those of bin g
__global__ void __launch_bounds__(TB) k_sel_hist(const Px* __restrict__ l0, Geo g, Params s, float* __restrict__ ths) {
    __shared__ int hist[50];
    if (threadIdx.x < 50) hist[threadIdx.x] = 0;
    __syncthreads();
    const int bx = blockIdx.x % g.w32, by = blockIdx.x / g.w32;
    for (int k = threadIdx.x; k < 32 * 32; k += TB) {
        const int it = (k & 31) + 32 * bx, jt = (k >> 5) + 32 * by;
        if (!edspix::hist_counted(it, jt, g.w, g.h)) continue;
        atomicAdd(&hist[edspix::hist_bin(l0[it + jt * g.w].pad) + 1], 1);
        atomicAdd(&hist[0], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) ths[blockIdx.x] = edspix::block_threshold(hist, s);
}

__global__ void __launch_bounds__(TB) k_sel_smooth(const float* __restrict__ ths, float* __restrict__ ths_s, int w32, int h32) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= w32 * h32) return;
    ths_s[i] = edspix::smooth_at(ths, w32, h32, i % w32, i / w32);
}

__global__ void __launch_bounds__(TB) k_sel_hits(Sel S, uint32_t* __restrict__ mask, int ns) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= ns) return;
    mask[i] = edspix::cell_mask(S, edspix::cell_of(S, i / SLOTS, i % SLOTS));
}

// n2 at the start of every cell, and whether the cell selects.  The two counts of a chunk travel in one int: certain selecting cells in
// the low half, ambiguous cells in the high half (1 024 at the most each).
__global__ void __launch_bounds__(SCAN) k_sel_scan(const uint32_t* __restrict__ mask, const uint8_t* __restrict__ table, int32_t* __restrict__ n2_start,
                                                   uint8_t* __restrict__ cell_sel, int32_t* __restrict__ counts, int ns, int wh) {
    __shared__ int wtot[SCAN / 64];
    __shared__ int P[SCAN], amb[SCAN], extra[SCAN + 1];
    __shared__ uint32_t ms[SCAN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base_c = 0, base_e = 0, amb_total = 0;
    for (int c0 = 0; c0 < ns; c0 += SCAN) {
        const int i = c0 + tid;
        const uint32_t m = i < ns ? mask[i] : 0u;
        const bool a = !edspix::mask_certain(m);
        const int v = (m == 0xFFFFu ? 1 : 0) | (a ? 1 << 16 : 0);
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int wbase = 0, total = 0;
        for (int k = 0; k < SCAN / 64; ++k) { if (k < wave) wbase += wtot[k]; total += wtot[k]; }
        const int excl = wbase + incl - v;
        const int Pi = excl & 0xFFFF, Ai = excl >> 16, nC = total & 0xFFFF, nA = total >> 16;
        P[tid] = Pi;
        ms[tid] = m;
        if (a) amb[Ai] = tid;
        __syncthreads();
        if (nA > 0 && tid == 0) {                       // serial in the ambiguous cells only
            int e = 0;
            extra[0] = 0;
            for (int k = 0; k < nA; ++k) {
                const int j = amb[k];
                e += edspix::cell_selected(ms[j], table, base_c + base_e + P[j] + e, wh);
                extra[k + 1] = e;
            }
        }
        __syncthreads();
        const int start = base_c + base_e + Pi + (nA > 0 ? extra[Ai] : 0);
        if (i < ns) {
            n2_start[i] = start;
            cell_sel[i] = (uint8_t)edspix::cell_selected(m, table, start, wh);
        }
        base_c += nC;
        base_e += nA > 0 ? extra[nA] : 0;
        amb_total += nA;
        __syncthreads();
    }
    if (tid == 0) { counts[C_N2] = base_c + base_e; counts[C_AMBIGUOUS] = amb_total; counts[C_N2_CERTAIN] = base_c; }
}

__global__ void __launch_bounds__(PICK) k_sel_pick(Sel S, const int32_t* __restrict__ n2_start, const uint8_t* __restrict__ cell_sel,
                                                   const uint8_t* __restrict__ table, uint8_t* __restrict__ map, int32_t* __restrict__ counts) {
    __shared__ Block B;
    __shared__ Key K[SLOTS + 5];
    const int b4 = blockIdx.x;
    if (threadIdx.x < SLOTS + 5) K[threadIdx.x] = 0;
    if (threadIdx.x == 0) edspix::make_block(S, b4, n2_start + (size_t)b4 * SLOTS, cell_sel + (size_t)b4 * SLOTS, table, B);
    __syncthreads();
    const int npx = B.bw * B.bh;
    for (int k = threadIdx.x; k < npx; k += PICK) {
        Key k2, k3, k4;
        const int slot = edspix::pixel_keys(S, B, k % B.bw, k / B.bw, &k2, &k3, &k4);
        if (k2) atomicMax(&K[slot], k2);
        if (k3) atomicMax(&K[SLOTS + (slot >> 2)], k3);
        if (k4) atomicMax(&K[SLOTS + 4], k4);
    }
    __syncthreads();
    if (threadIdx.x < SLOTS + 5) {
        const int v = edspix::finish_item(S, B, K, K + SLOTS, K + SLOTS + 4, threadIdx.x, map);
        if (v == 2) atomicAdd(&counts[C_N3], 1);
        if (v == 4) atomicAdd(&counts[C_N4], 1);
    }
}

__global__ void __launch_bounds__(TB) k_sel_count(const uint8_t* __restrict__ map, int32_t* __restrict__ block_cnt, int wh) {
    const int i = blockIdx.x * TB + threadIdx.x;
    const int c = __syncthreads_count(i < wh && map[i] != 0);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = c;
}

// The stable rank of the non-zero map pixels in flat order (blocks_before, then block_rank).  sub = 1: the sub-selection, pixel of rank rn is
// cleared when table[rn] > char_th, and what is left is counted per 256 into cnt_out.  sub = 0: the selection list.
__global__ void __launch_bounds__(TB) k_sel_rank(uint8_t* __restrict__ map, const int32_t* __restrict__ block_cnt, const uint8_t* __restrict__ table,
                                                 int sub, int char_th, int32_t* __restrict__ cnt_out, int32_t* __restrict__ uv, float* __restrict__ type,
                                                 int32_t* __restrict__ counts, int wh, int w) {
    __shared__ int s_wave[TB / 64];
    const int i = blockIdx.x * TB + threadIdx.x;
    const uint8_t v = i < wh ? map[i] : (uint8_t)0;              // in flight together with the counts blocks_before reads
    const bool nz = v != 0;
    const int base = edsdso::blocks_before<TB>(block_cnt, s_wave);
    int total;
    const int rank = base + edsdso::block_rank<TB>(nz, s_wave, &total);
    bool keep = nz;
    if (nz) {
        if (sub) {
            if (edspix::sub_removed(table, rank, char_th)) { map[i] = 0; keep = false; }
        } else {
            uv[2 * rank] = i % w; uv[2 * rank + 1] = i / w;
            type[rank] = (float)v;
        }
    }
    if (sub) {
        const int c = __syncthreads_count(keep);
        if (threadIdx.x == 0) cnt_out[blockIdx.x] = c;
    } else if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        counts[C_LIST] = base + total;
    }
}

// one select pass at `potential`; n[3] = n2, n3, n4 on the host
int select_pass(eds_sel* h, int potential, float thf, int32_t* n) {
    const Sel S = edspix::make_sel(h->lv[0], h->lv[1], h->lv[2], h->ths_s, h->g, h->prm, thf, potential);
    const int nb = S.nbx * S.nby, ns = nb * SLOTS, wh = h->W * h->H;
    if (ns > h->max_slots) return fail(EDS_ERR_INVALID, "select: more cells than the handle holds");
    EDS_HIP_TRY(hipMemsetAsync(h->map, 0, (size_t)wh, h->own.st));
    EDS_HIP_TRY(hipMemsetAsync(h->counts, 0, C_COUNTS * sizeof(int32_t), h->own.st));
    hipLaunchKernelGGL(k_sel_hits, dim3(blocks(ns)), dim3(TB), 0, h->own.st, S, h->mask, ns);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(SCAN), 0, h->own.st, h->mask, h->table, h->n2_start, h->cell_sel, h->counts, ns, wh);
    hipLaunchKernelGGL(k_sel_pick, dim3((unsigned)nb), dim3(PICK), 0, h->own.st, S, h->n2_start, h->cell_sel, h->table, h->map, h->counts);
    EDS_HIP_TRY(hipGetLastError());
    int32_t c[C_COUNTS];
    if (int rc = read_back(h->own, c, h->counts, sizeof(c))) return rc;
    n[0] = c[C_N2]; n[1] = c[C_N3]; n[2] = c[C_N4];
    h->ambiguous = c[C_AMBIGUOUS];
    h->n2_certain = c[C_N2_CERTAIN];
    return EDS_OK;
}

}  // namespace

extern "C" {

int eds_sel_abi_version(void) { return EDS_HIP_SELECT_ABI_VERSION; }

void eds_sel_params_default(eds_sel_params* p) {
    if (!p) return;
    const Params d = edspix::params_default();
    std::memcpy(p, &d, sizeof(d));
}

int eds_sel_create(int device, int H, int W, eds_sel** sel) {
    if (!sel) return fail(EDS_ERR_INVALID, "null output");
    *sel = nullptr;
    if (H < 32 || W < 32 || H > edspix::MAX_SIDE || W > edspix::MAX_SIDE) return fail(EDS_ERR_INVALID, "H and W are 32 .. 8192");
    eds_sel* h = new eds_sel;
    if (int rc = h->own.open(device)) { delete h; return rc; }
    h->H = H; h->W = W;
    h->g = edspix::make_geo(H, W);
    h->prm = edspix::params_default();
    h->max_slots = SLOTS * ((W + 3) / 4) * ((H + 3) / 4);          // potential 1
    const size_t px = (size_t)H * W, nt = (size_t)h->g.w32 * h->g.h32;
    h->n_blocks256 = (int)((px + TB - 1) / TB);
    const bool ok = h->own.alloc({{(void**)&h->lv[0], px * sizeof(Px)},
                                  {(void**)&h->lv[1], (size_t)h->g.w1 * h->g.h1 * sizeof(Px)},
                                  {(void**)&h->lv[2], (size_t)h->g.w2 * h->g.h2 * sizeof(Px)},
                                  {(void**)&h->in_img, px * sizeof(float)},
                                  {(void**)&h->B, 256 * sizeof(float)},
                                  {(void**)&h->ths, nt * sizeof(float)},
                                  {(void**)&h->ths_s, nt * sizeof(float)},
                                  {(void**)&h->map, px},
                                  {(void**)&h->table, px},
                                  {(void**)&h->mask, (size_t)h->max_slots * sizeof(uint32_t)},
                                  {(void**)&h->n2_start, (size_t)h->max_slots * sizeof(int32_t)},
                                  {(void**)&h->cell_sel, (size_t)h->max_slots},
                                  {(void**)&h->counts, C_COUNTS * sizeof(int32_t)},
                                  {(void**)&h->block_cnt, (size_t)2 * h->n_blocks256 * sizeof(int32_t)},
                                  {(void**)&h->uv, px * 2 * sizeof(int32_t)},
                                  {(void**)&h->type, px * sizeof(float)}}) &&
                    hipMemsetAsync(h->map, 0, px, h->own.st) == hipSuccess && hipStreamSynchronize(h->own.st) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        eds_sel_destroy(h);
        return fail(EDS_ERR_HIP, "eds_sel_create: the device refused a stream or an allocation");
    }
    *sel = h;
    return EDS_OK;
}

void eds_sel_destroy(eds_sel* h) {
    if (!h) return;
    h->own.close();
    delete h;
}

int eds_sel_set_params(eds_sel* h, const eds_sel_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null parameters");
    Params s;
    std::memcpy(&s, p, sizeof(s));
    if (!edspix::params_valid(s)) return fail(EDS_ERR_INVALID, "parameters: every float finite, min_grad_hist_cut 0 .. 1");
    h->prm = s;
    h->hist_valid = false;
    return EDS_OK;
}

int eds_sel_get_params(const eds_sel* h, eds_sel_params* p) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!p) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(p, &h->prm, sizeof(*p));
    return EDS_OK;
}

int eds_sel_set_random_pattern(eds_sel* h, const uint8_t* table, size_t n) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!table) return fail(EDS_ERR_INVALID, "table: NULL pointer");
    if (n != (size_t)h->W * h->H) return fail(EDS_ERR_INVALID, "the table holds W * H = " + std::to_string((size_t)h->W * h->H) + " bytes");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->table, table, n, hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->table_set = true;
    return EDS_OK;
}

int eds_sel_fill_reference_pattern(uint8_t* out, size_t n) {
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    edspix::fill_reference_pattern(out, n);
    return EDS_OK;
}

int eds_sel_set_potential(eds_sel* h, int potential) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (potential < 1 || potential > edspix::MAX_POTENTIAL) return fail(EDS_ERR_INVALID, "the potential is 1 .. 2^30");
    h->potential = potential;
    return EDS_OK;
}

int eds_sel_get_potential(const eds_sel* h, int* potential) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!potential) return fail(EDS_ERR_INVALID, "null output");
    *potential = h->potential;
    return EDS_OK;
}

int eds_sel_set_image(eds_sel* h, const float* image, int64_t rs, int on_device, const float* B) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    size_t bytes = 0;
    if (int rc = edscapi::check_image_layout(h->H, h->W, 1, image, &rs, nullptr, on_device, "image", nullptr, &bytes)) return rc;
    if (B)
        for (int i = 0; i < 256; ++i)
            if (!std::isfinite(B[i])) return fail(EDS_ERR_INVALID, "B is not finite");
    if (on_device)                                       // after B, as the checks have always run
        if (int rc = eds_dev_check_range(h->own.dev, image, bytes)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (int rc = edscapi::upload_image(h->own, h->in_img, h->H, h->W, image, rs, on_device)) return rc;
    if (B) EDS_HIP_TRY(hipMemcpyAsync(h->B, B, 256 * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    h->image_set = false;                               // what was stored is gone once the kernels are queued
    h->hist_valid = false;
    for (int l = 0; l < edspix::LEVELS; ++l) {
        const int w = edspix::level_w(h->g, l), hh = edspix::level_h(h->g, l);
        edscapi::queue_colours(h->own.st, l ? nullptr : h->in_img, l ? h->lv[l - 1] : nullptr, l ? edspix::level_w(h->g, l - 1) : 0, h->lv[l], w, hh);
        hipLaunchKernelGGL(k_sel_gradient, dim3(blocks((int64_t)w * hh)), dim3(TB), 0, h->own.st, h->lv[l], w, hh, B ? h->B : (const float*)nullptr);
    }
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->image_set = true;
    return EDS_OK;
}

int eds_sel_make_maps(eds_sel* h, float density, int recursions_left, float th_factor, int* num_have_sub, eds_sel_pass* passes, int max_passes,
                      int* n_passes, uint8_t* pass_maps) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!num_have_sub) return fail(EDS_ERR_INVALID, "null output");
    if (!(density > 0.0f) || !std::isfinite(density)) return fail(EDS_ERR_INVALID, "density is positive and finite");
    if (!(th_factor > 0.0f) || !std::isfinite(th_factor)) return fail(EDS_ERR_INVALID, "th_factor is positive and finite");
    if (recursions_left < 0) return fail(EDS_ERR_INVALID, "recursions_left >= 0");
    if (max_passes < 0 || (max_passes > 0 && !passes)) return fail(EDS_ERR_INVALID, "passes: max_passes entries");
    if (pass_maps && max_passes < 1) return fail(EDS_ERR_INVALID, "pass_maps comes with passes");
    if (!h->table_set) return fail(EDS_ERR_STATE, "no random pattern: eds_sel_set_random_pattern first");
    if (!h->image_set) return fail(EDS_ERR_STATE, "no image: eds_sel_set_image first");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const int wh = h->W * h->H, nt = h->g.w32 * h->g.h32;
    h->sel_valid = false;
    if (!h->hist_valid) {
        hipLaunchKernelGGL(k_sel_hist, dim3((unsigned)nt), dim3(TB), 0, h->own.st, h->lv[0], h->g, h->prm, h->ths);
        hipLaunchKernelGGL(k_sel_smooth, dim3(blocks(nt)), dim3(TB), 0, h->own.st, h->ths, h->ths_s, h->g.w32, h->g.h32);
        EDS_HIP_TRY(hipGetLastError());
        h->hist_valid = true;
    }
    std::vector<edspix::Pass> done;
    std::vector<uint8_t> maps;
    int np = 0;
    for (;;) {
        int32_t n[3];
        if (int rc = select_pass(h, h->potential, th_factor, n)) return rc;
        if (np < max_passes) {
            done.push_back(edspix::Pass{h->potential, n[0], n[1], n[2]});
            if (pass_maps) {
                maps.resize((size_t)(np + 1) * wh);
                if (int rc = read_back(h->own, maps.data() + (size_t)np * wh, h->map, (size_t)wh)) return rc;
            }
        }
        ++np;
        const edspix::Decision D = edspix::decide(n[0], n[1], n[2], density, recursions_left, h->potential);
        h->potential = D.new_potential;
        if (D.recurse) { --recursions_left; continue; }
        int32_t* cnt0 = h->block_cnt;
        int32_t* cnt1 = h->block_cnt + h->n_blocks256;
        hipLaunchKernelGGL(k_sel_count, dim3(blocks(wh)), dim3(TB), 0, h->own.st, h->map, cnt0, wh);
        if (D.subselect) {
            hipLaunchKernelGGL(k_sel_rank, dim3(blocks(wh)), dim3(TB), 0, h->own.st, h->map, cnt0, h->table, 1, D.char_th, cnt1, h->uv, h->type, h->counts,
                               wh, h->W);
            cnt0 = cnt1;
        }
        hipLaunchKernelGGL(k_sel_rank, dim3(blocks(wh)), dim3(TB), 0, h->own.st, h->map, cnt0, h->table, 0, 0, (int32_t*)nullptr, h->uv, h->type, h->counts,
                           wh, h->W);
        EDS_HIP_TRY(hipGetLastError());
        int32_t n_list = 0;
        if (int rc = read_back(h->own, &n_list, h->counts + C_LIST, sizeof(n_list))) return rc;
        h->n_sel = n_list;
        h->sel_valid = true;
        *num_have_sub = n_list;
        if (!done.empty()) std::memcpy(passes, done.data(), done.size() * sizeof(eds_sel_pass));
        if (pass_maps && !maps.empty()) std::memcpy(pass_maps, maps.data(), maps.size());
        if (n_passes) *n_passes = np;
        return EDS_OK;
    }
}

int eds_sel_get_map(eds_sel* h, uint8_t* out) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->sel_valid) return fail(EDS_ERR_STATE, "no selection: eds_sel_make_maps first");
    return read_back(h->own, out, h->map, (size_t)h->W * h->H);
}

int eds_sel_get_selection(eds_sel* h, int* n, int32_t* uv, float* type) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!n) return fail(EDS_ERR_INVALID, "null output");
    if (!h->sel_valid) return fail(EDS_ERR_STATE, "no selection: eds_sel_make_maps first");
    const size_t k = h->n_sel > 0 ? (size_t)h->n_sel : 0;
    if (int rc = read_back(h->own, uv, h->uv, k * 2 * sizeof(int32_t))) return rc;
    if (int rc = read_back(h->own, type, h->type, k * sizeof(float))) return rc;
    *n = h->n_sel;
    return EDS_OK;
}

int eds_sel_get_level(eds_sel* h, int lvl, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (lvl < 0 || lvl >= edspix::LEVELS) return fail(EDS_ERR_INVALID, "level 0 .. 2");
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->image_set) return fail(EDS_ERR_STATE, "no image: eds_sel_set_image first");
    const size_t n = (size_t)edspix::level_w(h->g, lvl) * edspix::level_h(h->g, lvl);
    return read_back(h->own, out, h->lv[lvl], n * sizeof(Px));
}

int eds_sel_get_thresholds(eds_sel* h, int which, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (which != EDS_SEL_THS && which != EDS_SEL_THS_SMOOTHED) return fail(EDS_ERR_INVALID, "which is EDS_SEL_THS or EDS_SEL_THS_SMOOTHED");
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->hist_valid) return fail(EDS_ERR_STATE, "no histograms: eds_sel_make_maps first");
    return read_back(h->own, out, which == EDS_SEL_THS ? h->ths : h->ths_s, (size_t)h->g.w32 * h->g.h32 * sizeof(float));
}

int eds_sel_get_scan_info(eds_sel* h, int* ambiguous_cells, int* n2_certain) {
    if (int rc = edscapi::check_handle(h, "eds_sel")) return rc;
    if (!h->sel_valid) return fail(EDS_ERR_STATE, "no selection: eds_sel_make_maps first");
    if (ambiguous_cells) *ambiguous_cells = h->ambiguous;
    if (n2_certain) *n2_certain = h->n2_certain;
    return EDS_OK;
}

}  // extern "C"
