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
// k_ini_nn: a query per lane walks the k-d tree nanoflann would build over the level (csrc/eds_nntree.hpp, shared with the host), so the
// table is the reference's, ties included.  The trees of the level and of the level above are built on the host from a read-back of their packed (u, v) and
// uploaded as nodes + vind; the walk's stack of pending far sides is private memory of the lane (no LDS).  A level whose tree is deeper than
// the stack — no level of lattice points is — gets its table from the host walk instead.
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

static_assert(NN_TILE == BLOCK, "the header's name for the queries of a workgroup");

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

// the points' (u, v) packed: what the host builds the level's tree from, and what the walk reads — 8 bytes a candidate, not a point's 64
__global__ void __launch_bounds__(BLOCK) k_ini_uv(const Pnt* __restrict__ p, int n, float2* __restrict__ uv) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) uv[i] = make_float2(p[i].u, p[i].v);
}

// one level's tree in device memory: nodes and vind as edsnn::build left them, uv the level's n points, box the root box
struct NnTree {
    const edsnn::Node* nodes;
    const int32_t* vind;
    const float* uv;
    edsnn::Box box;
    int n;
};

// makeNN for one level: out[n][NN_ROW].  A query per lane walks the level's tree for its ten neighbours and, with a level above
// (up.n > 0), that level's tree for its parent — edsnn::knn, the code the host runs, with its stack in the lane's private memory.
// The host launches this only for trees no deeper than edsnn::STACK.  Every index the walk follows was written by edsnn::build:
// nodes < 2 n, vind < n, a leaf's [left, right) inside [0, n].
__global__ void __launch_bounds__(BLOCK) k_ini_nn(const NnTree lvl, const NnTree up, int32_t* __restrict__ out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= lvl.n) return;
    const float q0 = lvl.uv[2 * (size_t)i], q1 = lvl.uv[2 * (size_t)i + 1];
    int32_t bi[edsini::NN];
    float bd[edsini::NN];
#pragma unroll
    for (int k = 0; k < edsini::NN; ++k) { bi[k] = -1; bd[k] = 0.0f; }
    edsnn::knn<edsini::NN>(lvl.nodes, lvl.vind, lvl.uv, lvl.box, q0, q1, bi, bd);
    int32_t parent = -1;
    if (up.n > 0) {
        float pd = 0.0f;
        edsnn::knn<1>(up.nodes, up.vind, up.uv, up.box, q0 * 0.5f - 0.25f, q1 * 0.5f - 0.25f, &parent, &pd);
        if (parent < 0) parent = 0;                            // no squared distance below FLT_MAX: edsini::make_nn's answer
    }
    int32_t* row = out + (size_t)i * NN_ROW;
#pragma unroll
    for (int k = 0; k < edsini::NN; ++k) row[k] = bi[k];
    row[edsini::NN] = parent;
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

// the set-up's device memory, at the first call that needs it
int setup_alloc(eds_ini* h) {
    if (h->status) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t lc = (size_t)h->geo.levels * h->cap;
    if (!h->own.alloc({{(void**)&h->status, (size_t)h->geo.total},
                       {(void**)&h->uv, lc * sizeof(float2)},
                       {(void**)&h->tree_nodes, 2 * 2 * (size_t)h->cap * sizeof(edsnn::Node)},
                       {(void**)&h->tree_vind, 2 * (size_t)h->cap * sizeof(int32_t)},
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

// a level's tree into slot 0 (the level) or 1 (the level above) of the handle's tree memory; the host arrays must outlive the copies
int upload_tree(eds_ini* h, int slot, const edsnn::Tree& t, const float2* uv, int n, NnTree* out) {
    edsnn::Node* nodes = h->tree_nodes + (size_t)slot * 2 * h->cap;
    int32_t* vind = h->tree_vind + (size_t)slot * h->cap;
    if (t.nodes.size() > 2 * (size_t)h->cap || t.vind.size() != (size_t)n) return fail(EDS_ERR_HIP, "eds_ini: a tree larger than its points allow");
    if (n > 0) {
        EDS_HIP_TRY(hipMemcpyAsync(nodes, t.nodes.data(), t.nodes.size() * sizeof(edsnn::Node), hipMemcpyHostToDevice, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(vind, t.vind.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
    }
    *out = NnTree{nodes, vind, reinterpret_cast<const float*>(uv), t.box, n};
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
    std::vector<float> uv(2 * (size_t)n + 2), uv_up(2 * (size_t)n_up + 2);
    edsnn::Tree tree, tree_up;
    h->nn_kernel_ms = 0.0f;
    bool on_device = false;
    if (n > 0) {
        SETUP_LAUNCH(h, k_ini_uv, edscapi::blocks(n, BLOCK), h->pts + o, n, h->uv + o);
        if (n_up > 0) SETUP_LAUNCH(h, k_ini_uv, edscapi::blocks(n_up, BLOCK), h->pts + o + h->cap, n_up, h->uv + o + h->cap);
        EDS_HIP_TRY(hipGetLastError());
        if (int rc = setup_read_back(h, uv.data(), h->uv + o, (size_t)n * sizeof(float2))) return rc;
        if (int rc = setup_read_back(h, uv_up.data(), h->uv + o + h->cap, (size_t)n_up * sizeof(float2))) return rc;
        edsnn::build(uv.data(), n, tree);
        edsnn::build(uv_up.data(), n_up, tree_up);
        on_device = tree.depth <= edsnn::STACK && tree_up.depth <= edsnn::STACK;
    }
    if (on_device) {
        NnTree d_lvl, d_up;
        if (int rc = upload_tree(h, 0, tree, h->uv + o, n, &d_lvl)) return rc;
        if (int rc = upload_tree(h, 1, tree_up, h->uv + o + h->cap, n_up, &d_up)) return rc;
        EDS_HIP_TRY(hipEventRecord(h->ev0, h->own.st));
        SETUP_LAUNCH(h, k_ini_nn, edscapi::blocks(n, BLOCK), d_lvl, d_up, h->nn + o * NN_ROW);
        EDS_HIP_TRY(hipEventRecord(h->ev1, h->own.st));
        EDS_HIP_TRY(hipGetLastError());
        if (int rc = setup_read_back(h, rows.data(), h->nn + o * NN_ROW, (size_t)n * NN_ROW * sizeof(int32_t))) return rc;
        if (hipEventElapsedTime(&h->nn_kernel_ms, h->ev0, h->ev1) != hipSuccess) { (void)hipGetLastError(); h->nn_kernel_ms = -1.0f; }
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < edsini::NN; ++k) nb[(size_t)i * edsini::NN + k] = rows[(size_t)i * NN_ROW + k];
            parent[i] = rows[(size_t)i * NN_ROW + edsini::NN];
        }
    } else if (n > 0) {
        // a tree deeper than the device walk's stack: the host walks (edsini::make_nn, by recursion) and the device gets the rows
        edsini::make_nn(n, uv.data(), n_up, uv_up.data(), nb.data(), n_up > 0 ? parent.data() : nullptr);
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < edsini::NN; ++k) rows[(size_t)i * NN_ROW + k] = nb[(size_t)i * edsini::NN + k];
            rows[(size_t)i * NN_ROW + edsini::NN] = n_up > 0 ? parent[i] : -1;
        }
        EDS_HIP_TRY(hipMemcpyAsync(h->nn + o * NN_ROW, rows.data(), (size_t)n * NN_ROW * sizeof(int32_t), hipMemcpyHostToDevice, h->own.st));
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
