// include/eds_hip_inisetup.h: the rest of CoarseInitializer::setFirst on the device — gridMaxSelection for makePixelStatus, makeNN, and
// the one call that runs the whole set-up.  The per-pixel rule, the cells, the tie order and makePixelStatus's controller are
// eds_inisetup.hpp, shared with the host; this file holds three kernels and the C entry points.  Built without contraction into FMAs
// (csrc/Makefile).
//
// k_grid_max: a cell per lane (G = 1, pot <= 8) or per wavefront (G = 64).  A lane visits the ranks lane, lane + G, ... of its cell in
// ascending order with the reference's strict >, so it holds the first of its largest scores; the wavefront form then folds the 64
// candidates under gms_better (larger score, then smaller rank), which is a total order on the candidates that have a score: the fold's
// winner is the serial loop's.  Cells are disjoint, so the cell's leader sets its pixels without a race and numGood is their number.
//
// k_ini_nn: a query per lane.  The candidates pass through LDS in tiles of NN_TILE, every lane reading the same address (a broadcast);
// the ten best stay in registers by an unrolled insertion under the total order (fp32 squared distance, index) of edsini::make_nn.
// Because that order is total the table does not depend on the order the candidates are visited in, and the kernel uses that twice:
// a workgroup starts at the tile of its own queries and walks outwards (the points are in row-major order, so near indices are near
// pixels and the ten best are nearly final after a few tiles), and a tile whose bounding box (k_ini_uv) is farther from every query
// of the workgroup than the query's tenth best is not read at all.  The box bound is formed with the candidates' own fp32 operations —
// the gap to the box squared and added, each rounding monotone — so it never exceeds the distance of a candidate inside the box.
// The parent is the same walk over the level above with one best.
//
// No kernel here waits on another workgroup, and every loop is bounded by a size passed in: nothing can spin.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_inisetup.h"
#include "eds_capi_internal.hpp"
#include "eds_init_internal.hpp"
#include "eds_inisetup.hpp"
#include "eds_pixsel_internal.hpp"

using edscapi::fail;
using edsct::Level;
using edsdso::Px;
using edsini::Pnt;

static_assert(edsini::NN == EDS_INI_NEIGHBOURS && edsini::SPARSITY_START == EDS_INI_SPARSITY_START, "header constants");

namespace {

constexpr int BLOCK = 256;
constexpr int NN_TILE = EDS_INI_NN_TILE;
constexpr int NN_ROW = edsini::NN + 1;                 // ten neighbours and the parent
constexpr int GMS_SERIAL_MAX_POT = 8;                  // up to here a lane walks its cell alone
constexpr float INF = __builtin_huge_valf();

static_assert(NN_TILE == BLOCK, "a lane stages one candidate of a tile");

// gridMaxSelection.  G lanes per cell; ncx x ncy cells; map is zero on entry; *count is zero on entry.
template <int G>
__global__ void __launch_bounds__(BLOCK) k_grid_max(const Px* __restrict__ grads, uint8_t* __restrict__ map, int w, int h, int pot, int ncx,
                                                    int ncy, float THFac, int32_t* __restrict__ count) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long cell = t / G;
    const int sub = (int)(t % G);
    const bool live = cell < (long long)ncx * ncy;
    float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int rank[4] = {-1, -1, -1, -1};
    size_t origin = 0;
    if (live) {
        const int x = 1 + (int)(cell % ncx) * pot, y = 1 + (int)(cell / ncx) * pot;       // x + pot < w and y + pot < h: every read is inside
        origin = (size_t)x + (size_t)y * w;
        const int cells = pot * pot;
        for (int r = sub; r < cells; r += G) {
            const int dx = r / pot, dy = r - dx * pot;
            float s[4];
            if (!edsini::gms_scores(grads[origin + dx + (size_t)dy * w], THFac, s)) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) if (s[k] > best[k]) { best[k] = s[k]; rank[k] = r; }
        }
    }
    if (G > 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float os = __shfl_xor(best[k], off);
                const int orank = __shfl_xor(rank[k], off);
                if (edsini::gms_better(os, orank, best[k], rank[k])) { best[k] = os; rank[k] = orank; }
            }
    }
    int good = 0;
    if (live && sub == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool first = rank[k] >= 0;
#pragma unroll
            for (int j = 0; j < k; ++j) first = first && rank[j] != rank[k];
            if (first) {
                const int dx = rank[k] / pot, dy = rank[k] - dx * pot;
                map[origin + dx + (size_t)dy * w] = 1;
                ++good;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) good += __shfl_xor(good, off);
    if ((threadIdx.x & 63) == 0 && good > 0) atomicAdd(count, good);
}

// the points' (u, v) packed — the search reads 8 bytes a candidate and not a point's 64 — and the bounding box of every tile of
// NN_TILE consecutive points: (min u, min v, max u, max v).  A workgroup per tile.
__global__ void __launch_bounds__(BLOCK) k_ini_uv(const Pnt* __restrict__ p, int n, float2* __restrict__ uv, float4* __restrict__ box) {
    __shared__ float4 part[BLOCK / 64];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    float4 b = make_float4(INF, INF, -INF, -INF);
    if (i < n) {
        const float2 c = make_float2(p[i].u, p[i].v);
        uv[i] = c;
        b = make_float4(c.x, c.y, c.x, c.y);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        b.x = fminf(b.x, __shfl_xor(b.x, off)); b.y = fminf(b.y, __shfl_xor(b.y, off));
        b.z = fmaxf(b.z, __shfl_xor(b.z, off)); b.w = fmaxf(b.w, __shfl_xor(b.w, off));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < BLOCK / 64; ++k) {
            b.x = fminf(b.x, part[k].x); b.y = fminf(b.y, part[k].y); b.z = fmaxf(b.z, part[k].z); b.w = fmaxf(b.w, part[k].w);
        }
        box[blockIdx.x] = b;
    }
}

// (d, j) before (bd, bi) in the total order: the smaller distance, then the lower index
__device__ __forceinline__ bool nn_before(float d, int32_t j, float bd, int32_t bi) { return d < bd || (d == bd && j < bi); }

// held (bd, bi) ascending in that order; (d, j) enters before the first held entry it precedes.  Constant indices only: registers.
__device__ __forceinline__ void nn_insert(float (&bd)[edsini::NN], int32_t (&bi)[edsini::NN], float d, int32_t j) {
#pragma unroll
    for (int k = edsini::NN - 1; k >= 1; --k) {
        const bool here = nn_before(d, j, bd[k], bi[k]), above = nn_before(d, j, bd[k - 1], bi[k - 1]);
        bi[k] = here ? (above ? bi[k - 1] : j) : bi[k];
        bd[k] = here ? (above ? bd[k - 1] : d) : bd[k];
    }
    if (nn_before(d, j, bd[0], bi[0])) { bd[0] = d; bi[0] = j; }
}

// what no candidate inside `box` can be nearer to (qx, qy) than: the gaps to the box through the candidates' own operations
__device__ __forceinline__ float nn_box_bound(float qx, float qy, const float4 box) {
    const float gx = fmaxf(fmaxf(box.x - qx, qx - box.z), 0.0f), gy = fmaxf(fmaxf(box.y - qy, qy - box.w), 0.0f);
    return gx * gx + gy * gy;
}

// the s-th tile of a walk outwards from tile `start`: start, start + 1, start - 1, ... with the side that ran out skipped
struct TileWalk {
    int lo, hi, ntiles, s;
    __device__ TileWalk(int start, int nt) : lo(start - 1), hi(start), ntiles(nt), s(0) {}
    __device__ bool more() const { return s < ntiles; }
    __device__ int next() {
        const bool up = hi < ntiles && (lo < 0 || (s & 1) == 0);
        ++s;
        return up ? hi++ : lo--;
    }
};

// one tile of `pts` (n of them) into LDS, two candidates to a float4; the places past the last point hold (inf, inf), whose distance is
// inf and never enters.  Every lane writes.
__device__ __forceinline__ void nn_stage(float4* tile, const float2* __restrict__ pts, int base, int n) {
    const int j = base + (int)threadIdx.x;
    reinterpret_cast<float2*>(tile)[threadIdx.x] = j < n ? pts[j] : make_float2(INF, INF);
}

// makeNN for one level: uv[n] its points with their tiles' boxes, up[n_up] those of the level above (n_up = 0 at the top level);
// out[n][NN_ROW].  A workgroup's queries are the points of tile blockIdx.x.  Four candidates a step: two 16-byte LDS reads, four
// distances, and one test of the nearest of them against the tenth best before any insertion is looked at.
__global__ void __launch_bounds__(BLOCK) k_ini_nn(const float2* __restrict__ uv, const float4* __restrict__ box, int n,
                                                  const float2* __restrict__ up, const float4* __restrict__ box_up, int n_up,
                                                  int32_t* __restrict__ out) {
    __shared__ float4 tile[NN_TILE / 2];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n;
    const float2 q = live ? uv[i] : make_float2(0.0f, 0.0f);
    const int ntiles = (n + NN_TILE - 1) / NN_TILE;
    float bd[edsini::NN];
    int32_t bi[edsini::NN];
#pragma unroll
    for (int k = 0; k < edsini::NN; ++k) { bd[k] = INF; bi[k] = -1; }
    for (TileWalk walk(blockIdx.x, ntiles); walk.more();) {
        const int t = walk.next(), base = t * NN_TILE;
        const bool need = live && nn_box_bound(q.x, q.y, box[t]) <= bd[edsini::NN - 1];
        if (!__syncthreads_or(need)) continue;                 // uniform; also the barrier before the tile is written again
        const int m = n - base < NN_TILE ? n - base : NN_TILE;
        nn_stage(tile, uv, base, n);
        __syncthreads();
        if (!__any(need)) continue;                            // this wavefront has nothing to find here
        for (int j = 0; j < m; j += 4) {                       // j <= NN_TILE - 4: the reads stay inside the tile
            const float4 a = tile[j >> 1], b = tile[(j >> 1) + 1];
            const float cx[4] = {a.x, a.z, b.x, b.z}, cy[4] = {a.y, a.w, b.y, b.w};
            float d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float d0 = q.x - cx[k], d1 = q.y - cy[k]; d[k] = d0 * d0 + d1 * d1; }
            if (!(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= bd[edsini::NN - 1])) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (nn_before(d[k], base + j + k, bd[edsini::NN - 1], bi[edsini::NN - 1])) nn_insert(bd, bi, d[k], base + j + k);
        }
    }
    int32_t parent = -1;
    if (n_up > 0) {
        const float qx = q.x * 0.5f - 0.25f, qy = q.y * 0.5f - 0.25f;
        const int ntiles_up = (n_up + NN_TILE - 1) / NN_TILE;
        float bestd = INF;
        for (TileWalk walk((int)((long long)blockIdx.x * ntiles_up / ntiles), ntiles_up); walk.more();) {
            const int t = walk.next(), base = t * NN_TILE;
            const bool need = live && nn_box_bound(qx, qy, box_up[t]) <= bestd;
            if (!__syncthreads_or(need)) continue;
            const int m = n_up - base < NN_TILE ? n_up - base : NN_TILE;
            nn_stage(tile, up, base, n_up);
            __syncthreads();
            if (!__any(need)) continue;
            for (int j = 0; j < m; j += 4) {
                const float4 a = tile[j >> 1], b = tile[(j >> 1) + 1];
                const float cx[4] = {a.x, a.z, b.x, b.z}, cy[4] = {a.y, a.w, b.y, b.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d0 = qx - cx[k], d1 = qy - cy[k], d = d0 * d0 + d1 * d1;
                    if (nn_before(d, base + j + k, bestd, parent)) { bestd = d; parent = base + j + k; }
                }
            }
        }
        if (parent < 0) parent = 0;                            // no finite distance: edsini::make_nn's answer
    }
    if (live) {
        int32_t* row = out + (size_t)i * NN_ROW;
#pragma unroll
        for (int k = 0; k < edsini::NN; ++k) row[k] = bi[k];
        row[edsini::NN] = parent;
    }
}

// every launch and wait of this file is counted on the handle, as eds_init.hip counts its own
#define SETUP_LAUNCH(h, kernel, grid, ...)                                                          \
    do {                                                                                            \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, (h)->own.st, __VA_ARGS__);           \
        ++(h)->n_launches;                                                                          \
    } while (0)

int setup_read_back(eds_ini* h, void* dst, const void* src, size_t bytes) {
    if (dst && bytes) ++h->n_waits;
    return edscapi::read_back(h->own, dst, src, bytes);
}

int check_level(const eds_ini* h, int lvl) {
    if (lvl < 0 || lvl >= h->geo.levels) return fail(EDS_ERR_INVALID, "level " + std::to_string(lvl) + " outside 0 .. " + std::to_string(h->geo.levels - 1));
    return EDS_OK;
}

size_t box_stride(const eds_ini* h) { return (size_t)(h->cap + NN_TILE - 1) / NN_TILE; }      // tiles of one level

// the set-up's device memory, at the first call that needs it
int setup_alloc(eds_ini* h) {
    if (h->status) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t lc = (size_t)h->geo.levels * h->cap;
    if (!h->own.alloc({{(void**)&h->status, (size_t)h->geo.total},
                       {(void**)&h->uv, lc * sizeof(float2)},
                       {(void**)&h->box, (size_t)h->geo.levels * box_stride(h) * sizeof(float4)},
                       {(void**)&h->nn, lc * NN_ROW * sizeof(int32_t)}}))
        return fail(EDS_ERR_HIP, "eds_ini: the device refused an allocation for the set-up");
    return EDS_OK;
}

// one gridMaxSelection of level lvl: the map cleared, the cells, the count back as one integer
int grid_pass(eds_ini* h, int lvl, int pot, float THFac, int* err) {
    const Level& L = h->geo.l[lvl];
    uint8_t* map = h->status + L.off;
    const int ncx = edsini::gms_cells(L.w, pot), ncy = edsini::gms_cells(L.h, pot);
    auto run = [&]() -> int {
        EDS_HIP_TRY(hipMemsetAsync(map, 0, (size_t)L.w * L.h, h->own.st));
        if (ncx < 1 || ncy < 1) return EDS_OK;
        EDS_HIP_TRY(hipMemsetAsync(h->d_count, 0, sizeof(int32_t), h->own.st));
        const long long cells = (long long)ncx * ncy;
        if (pot <= GMS_SERIAL_MAX_POT)
            SETUP_LAUNCH(h, k_grid_max<1>, edscapi::blocks(cells, BLOCK), h->first_px + L.off, map, L.w, L.h, pot, ncx, ncy, THFac, h->d_count);
        else
            SETUP_LAUNCH(h, k_grid_max<64>, edscapi::blocks(cells * 64, BLOCK), h->first_px + L.off, map, L.w, L.h, pot, ncx, ncy, THFac, h->d_count);
        EDS_HIP_TRY(hipGetLastError());
        return EDS_OK;
    };
    if ((*err = run())) return 0;
    int32_t n = 0;
    if (ncx >= 1 && ncy >= 1) *err = setup_read_back(h, &n, h->d_count, sizeof(n));
    return n;
}

int make_pixel_status(eds_ini* h, int lvl, float density, int recursions_left, float th_factor, int32_t* n_good_out, int32_t* passes_out) {
    if (int rc = setup_alloc(h)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    h->status_set[lvl] = false;
    int err = 0;
    int32_t sp = h->sparsity, passes = 0;
    const int n = edsini::make_pixel_status_ctl([&](int pot, float th, int* e) { return grid_pass(h, lvl, pot, th, e); }, density, recursions_left,
                                                th_factor, &sp, &passes, &err);
    if (err) return err;
    h->sparsity = sp;
    h->status_set[lvl] = true;
    if (n_good_out) *n_good_out = n;
    if (passes_out) *passes_out = passes;
    return EDS_OK;
}

int check_pixel_status_args(const eds_ini* h, int lvl, float density, int recursions_left, float th_factor) {
    if (int rc = check_level(h, lvl)) return rc;
    if (!(density > 0.0f) || !std::isfinite(density)) return fail(EDS_ERR_INVALID, "desired_density must be positive and finite");
    if (!(th_factor > 0.0f) || !std::isfinite(th_factor)) return fail(EDS_ERR_INVALID, "th_factor must be positive and finite");
    if (recursions_left < 0 || recursions_left > 64) return fail(EDS_ERR_INVALID, "recursions_left is 0 .. 64");
    if (!h->first_set) return fail(EDS_ERR_STATE, "eds_ini: no first frame set");
    return EDS_OK;
}

int check_neighbours_state(const eds_ini* h, int lvl) {
    const bool top = lvl == h->geo.levels - 1;
    if (!h->points_set[lvl] || (!top && !h->points_set[lvl + 1])) return fail(EDS_ERR_STATE, "eds_ini: the points of the level and of the level above come first");
    if (!top && h->n[lvl + 1] < 1) return fail(EDS_ERR_INVALID, "a parent table needs the points of the level above");
    return EDS_OK;
}

int make_neighbours(eds_ini* h, int lvl) {
    if (int rc = setup_alloc(h)) return rc;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const bool top = lvl == h->geo.levels - 1;
    const int n = h->n[lvl], n_up = top ? 0 : h->n[lvl + 1];
    const size_t o = (size_t)lvl * h->cap;
    h->nn_made[lvl] = false;
    std::vector<int32_t> rows((size_t)n * NN_ROW + 1), nb((size_t)n * edsini::NN + 1), parent((size_t)n + 1);
    h->nn_kernel_ms = 0.0f;
    if (n > 0) {
        const size_t ob = (size_t)lvl * box_stride(h), up = top ? 0 : 1;       // the level above is the next one in every array
        SETUP_LAUNCH(h, k_ini_uv, edscapi::blocks(n, BLOCK), h->pts + o, n, h->uv + o, h->box + ob);
        if (n_up > 0) SETUP_LAUNCH(h, k_ini_uv, edscapi::blocks(n_up, BLOCK), h->pts + o + h->cap, n_up, h->uv + o + h->cap, h->box + ob + box_stride(h));
        EDS_HIP_TRY(hipEventRecord(h->ev0, h->own.st));
        SETUP_LAUNCH(h, k_ini_nn, edscapi::blocks(n, BLOCK), h->uv + o, h->box + ob, n, h->uv + o + up * h->cap, h->box + ob + up * box_stride(h), n_up,
                     h->nn + o * NN_ROW);
        EDS_HIP_TRY(hipEventRecord(h->ev1, h->own.st));
        EDS_HIP_TRY(hipGetLastError());
        if (int rc = setup_read_back(h, rows.data(), h->nn + o * NN_ROW, (size_t)n * NN_ROW * sizeof(int32_t))) return rc;
        if (hipEventElapsedTime(&h->nn_kernel_ms, h->ev0, h->ev1) != hipSuccess) { (void)hipGetLastError(); h->nn_kernel_ms = -1.0f; }
    }
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < edsini::NN; ++k) nb[(size_t)i * edsini::NN + k] = rows[(size_t)i * NN_ROW + k];
        parent[i] = rows[(size_t)i * NN_ROW + edsini::NN];
    }
    if (int rc = eds_ini_set_neighbours(h, lvl, nb.data(), top ? nullptr : parent.data())) return rc;
    h->nn_made[lvl] = true;
    return EDS_OK;
}

}  // namespace

extern "C" {

int eds_ini_setup_abi_version(void) { return EDS_HIP_INISETUP_ABI_VERSION; }

int eds_ini_get_sparsity(const eds_ini* h, int32_t* out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    *out = h->sparsity;
    return EDS_OK;
}

int eds_ini_set_sparsity(eds_ini* h, int32_t value) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    h->sparsity = value < 1 ? 1 : value > edsini::SPARSITY_MAX ? edsini::SPARSITY_MAX : value;
    return EDS_OK;
}

int eds_ini_make_pixel_status(eds_ini* h, int lvl, float desired_density, int recursions_left, float th_factor, int32_t* n_good_out,
                              int32_t* passes_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_pixel_status_args(h, lvl, desired_density, recursions_left, th_factor)) return rc;
    return make_pixel_status(h, lvl, desired_density, recursions_left, th_factor, n_good_out, passes_out);
}

int eds_ini_get_pixel_status(eds_ini* h, int lvl, uint8_t* map_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (!map_out) return fail(EDS_ERR_INVALID, "null output");
    if (!h->status_set[lvl]) return fail(EDS_ERR_STATE, "eds_ini: the level has no pixel status (eds_ini_make_pixel_status first)");
    const Level& L = h->geo.l[lvl];
    return setup_read_back(h, map_out, h->status + L.off, (size_t)L.w * L.h);
}

int eds_ini_set_points_status(eds_ini* h, int lvl, int32_t* n_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (!h->status_set[lvl]) return fail(EDS_ERR_STATE, "eds_ini: the level has no pixel status (eds_ini_make_pixel_status first)");
    return edsini_internal::points_from_bytes(h, lvl, h->status + h->geo.l[lvl].off, n_out);
}

int eds_ini_make_neighbours(eds_ini* h, int lvl) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    if (int rc = check_neighbours_state(h, lvl)) return rc;
    return make_neighbours(h, lvl);
}

int eds_ini_get_neighbours(eds_ini* h, int lvl, int32_t* neighbours, int32_t* parent) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = check_level(h, lvl)) return rc;
    const bool top = lvl == h->geo.levels - 1;
    if (!neighbours || (!top && !parent)) return fail(EDS_ERR_INVALID, "neighbours (and, below the top level, parent) are required");
    if (!h->nn_made[lvl] || !h->tables_set[lvl]) return fail(EDS_ERR_STATE, "eds_ini: the level has no tables of eds_ini_make_neighbours");
    const int n = h->n[lvl];
    std::vector<int32_t> rows((size_t)n * NN_ROW + 1);
    if (int rc = setup_read_back(h, rows.data(), h->nn + (size_t)lvl * h->cap * NN_ROW, (size_t)n * NN_ROW * sizeof(int32_t))) return rc;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < edsini::NN; ++k) neighbours[(size_t)i * edsini::NN + k] = rows[(size_t)i * NN_ROW + k];
        if (!top) parent[i] = rows[(size_t)i * NN_ROW + edsini::NN];
    }
    return EDS_OK;
}

int eds_ini_get_neighbours_kernel_ms(const eds_ini* h, float* ms_out) {
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (!ms_out) return fail(EDS_ERR_INVALID, "null output");
    if (h->nn_kernel_ms < 0.0f) return fail(EDS_ERR_STATE, "eds_ini: eds_ini_make_neighbours has not run");
    *ms_out = h->nn_kernel_ms;
    return EDS_OK;
}

int eds_ini_setup_levels(eds_ini* h, eds_sel* sel, const float* densities, int32_t* n_out) {
    static const float reference[edsini::MAX_LEVELS] = {0.03f, 0.05f, 0.15f, 0.5f, 1.0f};       // :699
    if (int rc = edscapi::check_handle(h, "eds_ini")) return rc;
    if (int rc = edscapi::check_handle(sel, "eds_sel")) return rc;
    if (sel->H != h->geo.H || sel->W != h->geo.W || sel->own.dev != h->own.dev)
        return fail(EDS_ERR_INVALID, "the selector must be of the handle's H x W and on its device");
    const int levels = h->geo.levels;
    float density[edsini::MAX_LEVELS];
    for (int l = 0; l < levels; ++l) {
        const float d = densities ? densities[l] : reference[l];
        density[l] = (d * (float)h->geo.W) * (float)h->geo.H;                                    // :705-707
        if (!(density[l] > 0.0f) || !std::isfinite(density[l])) return fail(EDS_ERR_INVALID, "every density must be positive and finite");
    }
    if (!h->first_set) return fail(EDS_ERR_STATE, "eds_ini: no first frame set");
    if (!sel->image_set) return fail(EDS_ERR_STATE, "eds_sel: no image set (eds_sel_set_image with the first frame)");
    int32_t n[edsini::MAX_LEVELS] = {0, 0, 0, 0, 0};
    for (int l = 0; l < levels; ++l) {
        if (int rc = eds_sel_set_potential(sel, 3)) return rc;                                   // :702
        if (l == 0) {
            int have = 0;
            if (int rc = eds_sel_make_maps(sel, density[0], 1, 2.0f, &have, nullptr, 0, nullptr, nullptr)) return rc;
            if (int rc = eds_ini_set_points_selected(h, sel, &n[0])) return rc;
        } else {
            if (int rc = make_pixel_status(h, l, density[l], 5, 1.0f, nullptr, nullptr)) return rc;
            if (int rc = edsini_internal::points_from_bytes(h, l, h->status + h->geo.l[l].off, &n[l])) return rc;
        }
    }
    for (int l = levels - 1; l >= 0; --l) {
        if (int rc = check_neighbours_state(h, l)) return rc;
        if (int rc = make_neighbours(h, l)) return rc;
    }
    for (int l = 0; n_out && l < levels; ++l) n_out[l] = n[l];
    return EDS_OK;
}

}  // extern "C"
