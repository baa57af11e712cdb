// The keyframe switch for a range of slots without leaving the device (include/eds_hip_kfswitch.h):
//
//   k_kd_build      the depth map's k-d tree by sorting and partitioning (eds_kdbuild.hpp), one workgroup per map: eds_kdbuild_kernel.hpp,
//                   which an eds_imm's depth-seeded points (eds_immdepth.hip) launch too.  One flag per map: 0 built, 1 ambiguous, 2 more
//                   points than the launch holds.
//   the image kernels of eds_keyframe.hip (eds_keyframe_kernels.hpp) in their chunked form: one more grid dimension, counts read on the
//                   device, k_fill_slot_b filling only the slots the single call would have filled.
//
// A chunk of EDS_KFS_CHUNK slots is queued without a host wait — images, maps (copied, or projected by k_kfp_project into device memory),
// trees, selection, nearest points, weights, slots — then ONE wait reads the counts and flags.  A slot whose map was flagged is redone by
// eds_keyframe_build, i.e. exactly as eds_trk_build_keyframe does it, from the map downloaded out of the chunk's buffer.
//
// fp64 without FMA contraction (-ffp-contract=off, Makefile), fixed orders everywhere: a batch equals its singles bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/eds_hip_device.h"
#include "../../include/eds_hip_kfswitch.h"
#include "eds_capi_internal.hpp"
#include "eds_kdbuild.hpp"
#include "eds_kdbuild_kernel.hpp"
#include "eds_keyframe_kernels.hpp"

using namespace edscapi;

namespace {

constexpr int KFS_NB = 256;             // blocks of the min / max passes, as the single build

// the small per-chunk blocks, and the right of k_kd_build to its LDS
int ensure_small(eds_trk* h) {
    EdsKfsBuffers& k = h->kfs;
    if (!k.lds_set) {
        if (int rc = kd_build_reserve()) return rc;
        k.lds_set = true;
    }
    if (k.h_block) return EDS_OK;
    const size_t C = EDS_KFS_CHUNK, bytes = C * (4 + 16 + 32 + EDS_KFP_PAR * 8) + 64;
    char* dblock = nullptr;
    if (!h->own.alloc({mapped(k.h_block, dblock, bytes), {(void**)&k.d_mn, C * 4}, {(void**)&k.d_flag, C * 4}, {(void**)&k.d_summary, C * 16}, {(void**)&k.d_K, C * 32}}))
        return fail(EDS_ERR_HIP, "allocation of the keyframe switch's blocks failed");
    k.h_par = reinterpret_cast<double*>(k.h_block);                    // doubles first: every part stays aligned
    k.d_par = reinterpret_cast<double*>(dblock);
    k.h_K = k.h_par + C * EDS_KFP_PAR;
    k.h_summary = reinterpret_cast<int*>(k.h_K + C * 4);
    k.h_mn = k.h_summary + C * 4;
    return EDS_OK;
}

int ensure_maps(eds_trk* h, size_t stride) {
    EdsKfsBuffers& k = h->kfs;
    if (stride < 1) stride = 1;
    if (k.d_mxy && k.map_stride >= stride) return EDS_OK;
    const size_t n = stride * EDS_KFS_CHUNK;
    if (!h->own.regrow(k.map_stride, stride, {{(void**)&k.d_mxy, n * 16}, {(void**)&k.d_midp, n * 8}, {(void**)&k.d_txy, n * 16}, {(void**)&k.d_tidp, n * 8},
                                             {(void**)&k.d_msrc, n * 4}, {(void**)&k.d_perm, n * 4}}))
        return fail(EDS_ERR_HIP, "allocation of the keyframe switch's map buffers failed");
    return EDS_OK;
}

size_t cell_stride_of(const eds_trk* h) { return (size_t)h->H * h->W / 4 + 2; }       // cells are at least 2 x 2

int ensure_images(eds_trk* h, bool outputs) {
    EdsKfsBuffers& k = h->kfs;
    const size_t C = EDS_KFS_CHUNK, n = (size_t)h->H * h->W * C, cs = cell_stride_of(h) * C;
    if (!k.d_raw) {
        if (!h->own.alloc({{&k.d_raw, n * 8}, {(void**)&k.d_log, n * 8}, {(void**)&k.d_gx, n * 8}, {(void**)&k.d_gy, n * 8}, {(void**)&k.d_mag, n * 8},
                           {(void**)&k.d_idp, n * 8}, {(void**)&k.d_w, n * 8}, {(void**)&k.d_coord, n * 16}, {(void**)&k.d_grad, n * 16},
                           {(void**)&k.d_partial, C * 2 * KFS_NB * 8}, {(void**)&k.d_cand, n * 4}, {(void**)&k.d_cnt, cs * 4}, {(void**)&k.d_off, cs * 4}}))
            return fail(EDS_ERR_HIP, "allocation of the keyframe switch's image buffers failed");
    }
    if (outputs && !k.h_out) {
        k.out_n = std::min((size_t)h->Np, (size_t)h->H * h->W);
        if (!h->own.alloc_pinned(k.h_out, C * 6 * k.out_n * 8)) return fail(EDS_ERR_HIP, "allocation of the keyframe switch's output staging failed");
    }
    return EDS_OK;
}

int launch_trees(eds_trk* h, int cn, const double* d_xy, const double* d_idp, size_t in_stride, int max_m, size_t out_stride, double* d_txy,
                 double* d_tidp) {
    EdsKfsBuffers& k = h->kfs;
    return kd_build_launch(h->own.st, cn, d_xy, d_idp, in_stride, k.d_mn, max_m, out_stride, k.d_perm, d_txy, d_tidp, k.d_flag);
}

struct Images {
    const void* const* host = nullptr;      // count host pointers, or
    const void* dev = nullptr;              // device memory with strides in elements
    int64_t frame_stride = 0, row_stride = 0;
};

int build_keyframes(eds_trk* h, int first, int count, int img_type, const Images& im, const eds_kf_select* sel, const double* K,
                    const eds_kfs_depth* depth, const eds_kfs_out* out) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (!sel) return fail(EDS_ERR_INVALID, "null selection parameters");
    if (!K && !(depth && depth->source == EDS_KFS_DEPTH_SLOTS)) return fail(EDS_ERR_INVALID, "null intrinsics (NULL: the source slots' own, with EDS_KFS_DEPTH_SLOTS only)");
    if (img_type < 0 || img_type > 2) return fail(EDS_ERR_INVALID, "img_type must be EDS_IMG_U8, EDS_IMG_F32 or EDS_IMG_F64");
    const int H = h->H, W = h->W, cell = sel->cell;
    const size_t npx = (size_t)H * W, px = img_type == 0 ? 1 : (img_type == 1 ? 4 : 8);
    if (cell < 2 || cell > KF_MAX_CELL || cell > H || cell > W) return fail(EDS_ERR_INVALID, "cell size must be in [2, 32] and fit the image");
    if (sel->method != EDS_KF_MAX && sel->method != EDS_KF_MEDIAN) return fail(EDS_ERR_INVALID, "unknown point selection method");
    int64_t fs = im.frame_stride, rs = im.row_stride;
    if (im.host) {
        for (int b = 0; b < count; ++b) if (!im.host[b]) return fail(EDS_ERR_INVALID, "null image");
    } else {
        if (rs == 0) rs = W;
        if (fs == 0) fs = (int64_t)(H - 1) * rs + W;
        if (rs < W || fs < (int64_t)(H - 1) * rs + W || fs > (int64_t)1 << 40)
            return fail(EDS_ERR_INVALID, "bad strides: row_stride >= W and frame_stride >= (H - 1) * row_stride + W, in elements (0 = dense)");
        if (!im.dev || (reinterpret_cast<uintptr_t>(im.dev) & (px - 1))) return fail(EDS_ERR_INVALID, "d_images is null or not aligned to its element size");
    }
    const int source = depth ? depth->source : EDS_KFS_DEPTH_NONE;
    if (source < EDS_KFS_DEPTH_NONE || source > EDS_KFS_DEPTH_SLOTS) return fail(EDS_ERR_INVALID, "unknown depth source");
    const bool arrays = source == EDS_KFS_DEPTH_HOST || source == EDS_KFS_DEPTH_DEVICE;
    int64_t max_n = 0, extent = 0;
    if (arrays) {
        if (!depth->n) return fail(EDS_ERR_INVALID, "null depth-map sizes");
        for (int b = 0; b < count; ++b) {
            if (depth->n[b] < 0) return fail(EDS_ERR_INVALID, "negative depth-map size");
            max_n = std::max<int64_t>(max_n, depth->n[b]);
        }
        if (max_n > 0) {
            if (!depth->depth_xy || !depth->depth_idp) return fail(EDS_ERR_INVALID, "null depth map");
            if (depth->stride < max_n || depth->stride > (int64_t)1 << 40) return fail(EDS_ERR_INVALID, "depth stride must be at least the largest n");
            for (int b = 0; b < count; ++b) if (depth->n[b] > 0) extent = std::max<int64_t>(extent, b * depth->stride + depth->n[b]);
        }
    } else if (source == EDS_KFS_DEPTH_SLOTS) {
        const int sf = depth->src_first;
        if ((rc = check_range(h, sf, count))) return rc;
        if (sf != first && sf < first + count && first < sf + count)
            return fail(EDS_ERR_INVALID, "source and destination slots overlap: src_first == first (in place) or disjoint ranges");
        if ((rc = eds_kfp_check_transforms(count, depth->T7, depth->K_dst))) return rc;
    }
    const bool vectors = out && (out->coord_xy || out->norm_xy || out->grad_xy || out->idp || out->weights);
    if (vectors && out->stride < h->Nmax) return fail(EDS_ERR_INVALID, "output stride smaller than the handle's max_points");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (!im.host && (rc = eds_dev_check_range(h->own.dev, im.dev, (size_t)((count - 1) * fs + (int64_t)(H - 1) * rs + W) * px))) return rc;
    if (source == EDS_KFS_DEPTH_DEVICE && max_n > 0) {
        if ((reinterpret_cast<uintptr_t>(depth->depth_xy) | reinterpret_cast<uintptr_t>(depth->depth_idp)) & 7)
            return fail(EDS_ERR_INVALID, "a depth-map array is not aligned to a double");
        if ((rc = eds_dev_check_range(h->own.dev, depth->depth_xy, (size_t)extent * 16))) return rc;
        if ((rc = eds_dev_check_range(h->own.dev, depth->depth_idp, (size_t)extent * 8))) return rc;
    }
    if ((rc = check_idle_slots(h, first, count, 0))) return rc;
    if (source == EDS_KFS_DEPTH_SLOTS && (rc = check_idle_slots(h, depth->src_first, count, EDS_NEED_KF))) return rc;
    if ((rc = ensure_small(h))) return rc;
    const size_t ms = source == EDS_KFS_DEPTH_SLOTS ? (size_t)h->Np : (size_t)std::max<int64_t>(max_n, 1);
    if ((rc = ensure_maps(h, ms))) return rc;
    if ((rc = ensure_images(h, vectors))) return rc;
    EdsKfsBuffers& k = h->kfs;
    h->kf_build.last_slot = -1;               // eds_trk_get_keyframe_points speaks of the single build's last slot only
    hipStream_t st = h->own.st;
    const size_t cs = cell_stride_of(h);
    const int ncx = W / cell, ncy = H / cell, ncell = ncx * ncy, n2 = cell * cell;       // only whole cells (KeyFrame.cpp:752-754)
    const int k_per_cell = sel->method == EDS_KF_MAX ? (sel->num_points > 0 ? sel->num_points / ncell : 0) : 0;
    const size_t cand_bound = (size_t)ncell * (sel->method == EDS_KF_MAX ? std::min(k_per_cell, n2) : n2);
    const double const_idp = 1.0 / ((sel->max_depth - sel->min_depth) / 2.0);       // KeyFrame.cpp:1189
    std::vector<unsigned char> h_img;
    std::vector<double> h_xy, h_idp;
    int result = EDS_OK;
    for (int c0 = 0; c0 < count; c0 += EDS_KFS_CHUNK) {
        const int cn = std::min(EDS_KFS_CHUNK, count - c0);
        // ---- queue: images
        for (int b = 0; b < cn; ++b) {
            char* dst = static_cast<char*>(k.d_raw) + (size_t)b * npx * 8;
            if (im.host) EDS_HIP_TRY(hipMemcpyAsync(dst, im.host[c0 + b], npx * px, hipMemcpyHostToDevice, st));
            else EDS_HIP_TRY(hipMemcpy2DAsync(dst, (size_t)W * px, static_cast<const char*>(im.dev) + (size_t)(c0 + b) * fs * px, (size_t)rs * px,
                                              (size_t)W * px, H, hipMemcpyDeviceToDevice, st));
        }
        // ---- the maps and their trees
        int max_m = 0;
        if (source == EDS_KFS_DEPTH_SLOTS) {
            const int sf = depth->src_first + c0;
            max_m = max_points(h, sf, cn);
            if ((rc = eds_kfp_project_queue(h, sf, cn, depth->T7 ? depth->T7 + 7 * (size_t)c0 : nullptr, depth->K_dst ? depth->K_dst + 4 * (size_t)c0 : nullptr,
                                            (double)W, (double)H, k.h_par, k.d_par, k.d_mn, k.d_mxy, k.d_midp, k.d_msrc))) return rc;
        } else {
            for (int b = 0; b < cn; ++b) {
                const int n = arrays ? depth->n[c0 + b] : 0;
                k.h_mn[b] = n;
                max_m = std::max(max_m, n);
                if (n < 1) continue;
                const size_t o = (size_t)(c0 + b) * depth->stride;
                const hipMemcpyKind kind = source == EDS_KFS_DEPTH_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
                EDS_HIP_TRY(hipMemcpyAsync(k.d_mxy + 2 * ms * b, depth->depth_xy + 2 * o, (size_t)n * 16, kind, st));
                EDS_HIP_TRY(hipMemcpyAsync(k.d_midp + ms * b, depth->depth_idp + o, (size_t)n * 8, kind, st));
            }
            EDS_HIP_TRY(hipMemcpyAsync(k.d_mn, k.h_mn, (size_t)cn * 4, hipMemcpyHostToDevice, st));
        }
        if ((rc = launch_trees(h, cn, k.d_mxy, k.d_midp, ms, max_m, ms, k.d_txy, k.d_tidp))) return rc;
        // ---- the image side, as eds_keyframe_build queues it for one slot
        for (int b = 0; b < cn; ++b) std::memcpy(k.h_K + 4 * b, K ? K + 4 * (size_t)(c0 + b) : h->slots[depth->src_first + c0 + b].K, 32);
        EDS_HIP_TRY(hipMemcpyAsync(k.d_K, k.h_K, (size_t)cn * 32, hipMemcpyHostToDevice, st));
        const dim3 T(KF_T);
        hipLaunchKernelGGL(k_minmax_b, dim3(KFS_NB, cn), T, 0, st, (const void*)k.d_raw, npx * 8, img_type, npx, k.d_partial, 2 * KFS_NB);
        hipLaunchKernelGGL(k_log_b, dim3(KFS_NB, cn), T, 0, st, (const void*)k.d_raw, npx * 8, img_type, npx, (const double*)k.d_partial, 2 * KFS_NB, KFS_NB,
                           k.d_log);
        hipLaunchKernelGGL(k_sobel_b, dim3((W + KF_T - 1) / KF_T, H, cn), T, 0, st, (int)sel->sobel_ksize, (const double*)k.d_log, H, W, k.d_gx, k.d_gy, k.d_mag);
        hipLaunchKernelGGL(k_select_b, dim3(ncell, cn), T, 0, st, (const double*)k.d_mag, npx, W, cell, ncx, (int)sel->method, k_per_cell, k.d_cand, k.d_cnt,
                           (int)cs);
        hipLaunchKernelGGL(k_scan_cells_b, dim3(cn), T, 0, st, (const int*)k.d_cnt, ncell, k.d_off, (int)cs);
        hipLaunchKernelGGL(k_emit_b, dim3(ncell, cn), T, 0, st, (const int*)k.d_cand, (const int*)k.d_cnt, (const int*)k.d_off, (int)cs, npx, cell, ncx, W,
                           (const double*)k.d_gx, (const double*)k.d_gy, k.d_coord, k.d_grad);
        const int* d_ncand = k.d_off + ncell;                 // slot b's candidate count: d_ncand[b * cs]
        if (max_m > 0 && cand_bound > 0) {
            hipLaunchKernelGGL(k_nearest_tree_b, dim3((unsigned)((cand_bound + KF_T - 1) / KF_T), cn), T, 0, st, (const double*)k.d_coord, npx, d_ncand, (int)cs,
                               (const double*)k.d_txy, (const double*)k.d_tidp, ms, (const int*)k.d_mn, (const int*)k.d_flag, k.d_idp, k.d_w);
            hipLaunchKernelGGL(k_minmax_counted_b, dim3(KFS_NB, cn), T, 0, st, (const double*)k.d_w, npx, d_ncand, (int)cs, k.d_partial, 2 * KFS_NB);
        }
        hipLaunchKernelGGL(k_weights_clean_b, dim3(cn), dim3(1024), 0, st, k.d_coord, k.d_grad, k.d_idp, k.d_w, npx, d_ncand, (int)cs, (const int*)k.d_mn,
                           (const int*)k.d_flag, const_idp, (const double*)k.d_partial, 2 * KFS_NB, KFS_NB, sel->weight_threshold, k.d_summary);
        hipLaunchKernelGGL(k_fill_slot_b, dim3(h->Np / KF_T, cn), T, 0, st, h->arrays(), first + c0, h->Nmax, (const double*)k.d_K, (const int*)k.d_summary,
                           npx, (const double*)k.d_coord, (const double*)k.d_grad, (const double*)k.d_idp, (const double*)k.d_w);
        EDS_HIP_TRY(hipGetLastError());
        EDS_HIP_TRY(hipMemcpyAsync(k.h_summary, k.d_summary, (size_t)cn * 16, hipMemcpyDeviceToHost, st));
        if (vectors) {
            const size_t on = k.out_n;
            for (int b = 0; b < cn; ++b) {
                double* o = k.h_out + (size_t)b * 6 * on;
                EDS_HIP_TRY(hipMemcpyAsync(o, k.d_coord + 2 * npx * b, on * 16, hipMemcpyDeviceToHost, st));
                EDS_HIP_TRY(hipMemcpyAsync(o + 2 * on, k.d_grad + 2 * npx * b, on * 16, hipMemcpyDeviceToHost, st));
                EDS_HIP_TRY(hipMemcpyAsync(o + 4 * on, k.d_idp + npx * b, on * 8, hipMemcpyDeviceToHost, st));
                EDS_HIP_TRY(hipMemcpyAsync(o + 5 * on, k.d_w + npx * b, on * 8, hipMemcpyDeviceToHost, st));
            }
        }
        // ---- the chunk's one wait
        EDS_HIP_TRY(hipStreamSynchronize(st));
        for (int b = 0; b < cn; ++b) {
            const int g = c0 + b, slot = first + g;
            const int ncand = k.h_summary[4 * b], N = k.h_summary[4 * b + 1], m = k.h_summary[4 * b + 2], flag = k.h_summary[4 * b + 3];
            const double* Kb = k.h_K + 4 * b;
            int code = EDS_OK, np = -1;
            if (out && out->tree_on_host) out->tree_on_host[g] = flag != 0 ? 1 : 0;
            if (flag != 0) {
                // ambiguous or beyond the capacity: this slot exactly as eds_trk_build_keyframe does it, its map taken back from the device
                const void* img = im.host ? im.host[g] : nullptr;
                if (!im.host) {
                    h_img.resize(npx * px);
                    EDS_HIP_TRY(hipMemcpy2D(h_img.data(), (size_t)W * px, static_cast<const char*>(im.dev) + (size_t)g * fs * px, (size_t)rs * px,
                                            (size_t)W * px, H, hipMemcpyDeviceToHost));
                    img = h_img.data();
                }
                const double *mxy, *midp;
                if (source == EDS_KFS_DEPTH_HOST) {
                    mxy = depth->depth_xy + 2 * (size_t)g * depth->stride; midp = depth->depth_idp + (size_t)g * depth->stride;
                } else {
                    h_xy.resize(2 * (size_t)m); h_idp.resize(m);
                    EDS_HIP_TRY(hipMemcpy(h_xy.data(), k.d_mxy + 2 * ms * b, (size_t)m * 16, hipMemcpyDeviceToHost));
                    EDS_HIP_TRY(hipMemcpy(h_idp.data(), k.d_midp + ms * b, (size_t)m * 8, hipMemcpyDeviceToHost));
                    mxy = h_xy.data(); midp = h_idp.data();
                }
                code = eds_keyframe_build(h, slot, img_type, img, H, W, 1, sel, m, mxy, midp, Kb[0], Kb[1], Kb[2], Kb[3], &np);
                if (code == EDS_OK && vectors) {
                    const size_t o = (size_t)g * out->stride;
                    code = eds_keyframe_get_points(h, slot, out->coord_xy ? out->coord_xy + 2 * o : nullptr, out->norm_xy ? out->norm_xy + 2 * o : nullptr,
                                                   out->grad_xy ? out->grad_xy + 2 * o : nullptr, out->idp ? out->idp + o : nullptr,
                                                   out->weights ? out->weights + o : nullptr);
                }
                h->kf_build.last_slot = -1;
            } else if (ncand < 1) {
                code = fail(EDS_ERR_INVALID, "the selection produced no candidate point");
            } else {
                np = N;
                if (N < 1) code = fail(EDS_ERR_INVALID, "no point survived the weight threshold");
                else if (N > h->Nmax) code = fail(EDS_ERR_INVALID, "the keyframe has more points than the handle's max_points");
            }
            if (flag == 0 && code == EDS_OK) {             // the planes are filled (k_fill_slot_b): the host side of eds_keyframe_build's end
                Slot& s = h->slots[slot];
                s.N = N; s.K[0] = Kb[0]; s.K[1] = Kb[1]; s.K[2] = Kb[2]; s.K[3] = Kb[3];
                s.num_points = ncand;
                if ((code = refresh_gram(h, slot, false)) == EDS_OK) {
                    s.has_kf = true;
                    s.seeded = false;
                    eds_klt_reset_slot(h, slot);
                    s.epi_valid = false;
                    s.residuals.clear();
                    s.res_on_device = false; s.trace_on_device = false; s.ntrace = 0;
                    if (vectors) {
                        const size_t on = k.out_n, o = (size_t)g * out->stride;
                        const double* src = k.h_out + (size_t)b * 6 * on;
                        if (out->coord_xy) std::memcpy(out->coord_xy + 2 * o, src, (size_t)N * 16);
                        for (int i = 0; out->norm_xy && i < N; ++i) {              // KeyFrame.cpp:417-423
                            out->norm_xy[2 * (o + i)] = (src[2 * i] - Kb[2]) / Kb[0];
                            out->norm_xy[2 * (o + i) + 1] = (src[2 * i + 1] - Kb[3]) / Kb[1];
                        }
                        if (out->grad_xy) std::memcpy(out->grad_xy + 2 * o, src + 2 * on, (size_t)N * 16);
                        if (out->idp) std::memcpy(out->idp + o, src + 4 * on, (size_t)N * 8);
                        if (out->weights) std::memcpy(out->weights + o, src + 5 * on, (size_t)N * 8);
                    }
                }
            }
            if (out && out->n_points && np >= 0) out->n_points[g] = np;
            if (out && out->status) out->status[g] = code;
            if (code != EDS_OK && result == EDS_OK) result = code;
        }
    }
    return result;
}

}  // namespace

extern "C" {

int eds_kfs_abi_version(void) { return EDS_HIP_KFSWITCH_ABI_VERSION; }
int eds_kfs_tree_capacity(void) { return edskdb::CAPACITY; }
int eds_kfs_chunk_size(void) { return EDS_KFS_CHUNK; }

int eds_kfs_build_tree(eds_trk* h, int count, const int* n, const double* d_depth_xy, int64_t stride, int32_t* perm_out, uint8_t* on_host_out) {
    if (!h) return fail(EDS_ERR_INVALID, "null handle");
    if (count < 1 || !n || !perm_out) return fail(EDS_ERR_INVALID, "bad count, or null sizes or output");
    int64_t max_n = 0, extent = 0;
    for (int b = 0; b < count; ++b) {
        if (n[b] < 0) return fail(EDS_ERR_INVALID, "negative depth-map size");
        max_n = std::max<int64_t>(max_n, n[b]);
    }
    if (stride < std::max<int64_t>(max_n, 1) || stride > (int64_t)1 << 40) return fail(EDS_ERR_INVALID, "stride must be at least the largest n");
    for (int b = 0; b < count; ++b) if (n[b] > 0) extent = std::max<int64_t>(extent, b * stride + n[b]);
    if (reinterpret_cast<uintptr_t>(d_depth_xy) & 7) return fail(EDS_ERR_INVALID, "d_depth_xy is not aligned to a double");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    int rc;
    if (extent > 0 && (rc = eds_dev_check_range(h->own.dev, d_depth_xy, (size_t)extent * 16))) return rc;
    if (h->fused.pending_count > 0) return fail(EDS_ERR_STATE, "a batch is in flight: call eds_trk_sync first");
    if (extent == 0) { if (on_host_out) std::memset(on_host_out, 0, count); return EDS_OK; }
    if ((rc = ensure_small(h))) return rc;
    const size_t ps = (size_t)std::min<int64_t>(max_n, edskdb::CAPACITY);        // the permutations' stride on the device
    if ((rc = ensure_maps(h, ps))) return rc;
    EdsKfsBuffers& k = h->kfs;
    std::vector<int> perm((size_t)EDS_KFS_CHUNK * ps);
    std::vector<double> xy;
    int flags[EDS_KFS_CHUNK];
    for (int c0 = 0; c0 < count; c0 += EDS_KFS_CHUNK) {
        const int cn = std::min(EDS_KFS_CHUNK, count - c0);
        int max_m = 0;
        for (int b = 0; b < cn; ++b) { k.h_mn[b] = n[c0 + b]; max_m = std::max(max_m, n[c0 + b]); }
        EDS_HIP_TRY(hipMemcpyAsync(k.d_mn, k.h_mn, (size_t)cn * 4, hipMemcpyHostToDevice, h->own.st));
        if ((rc = launch_trees(h, cn, d_depth_xy + 2 * (size_t)c0 * stride, nullptr, (size_t)stride, max_m, ps, nullptr, nullptr))) return rc;
        EDS_HIP_TRY(hipMemcpyAsync(flags, k.d_flag, (size_t)cn * 4, hipMemcpyDeviceToHost, h->own.st));
        EDS_HIP_TRY(hipMemcpyAsync(perm.data(), k.d_perm, (size_t)cn * ps * 4, hipMemcpyDeviceToHost, h->own.st));
        EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
        for (int b = 0; b < cn; ++b) {
            const int m = n[c0 + b];
            int32_t* dst = perm_out + (size_t)(c0 + b) * stride;
            if (on_host_out) on_host_out[c0 + b] = flags[b] != 0 ? 1 : 0;
            if (flags[b] == 0) { if (m > 0) std::memcpy(dst, perm.data() + (size_t)b * ps, (size_t)m * 4); continue; }
            xy.resize(2 * (size_t)m);
            EDS_HIP_TRY(hipMemcpy(xy.data(), d_depth_xy + 2 * (size_t)(c0 + b) * stride, (size_t)m * 16, hipMemcpyDeviceToHost));
            edskd::build_tree(xy.data(), m, dst);
        }
    }
    return EDS_OK;
}

int eds_kfs_build_keyframes(eds_trk* h, int first, int count, int img_type, const void* const* images, const eds_kf_select* sel,
                            const double* K, const eds_kfs_depth* depth, const eds_kfs_out* out) {
    int rc = check_range(h, first, count);
    if (rc) return rc;
    if (!images) return fail(EDS_ERR_INVALID, "null images");
    Images im;
    im.host = images;
    return build_keyframes(h, first, count, img_type, im, sel, K, depth, out);
}

int eds_kfs_build_keyframes_dev(eds_trk* h, int first, int count, int img_type, const void* d_images, int64_t frame_stride,
                                int64_t row_stride, const eds_kf_select* sel, const double* K, const eds_kfs_depth* depth,
                                const eds_kfs_out* out) {
    Images im;
    im.dev = d_images; im.frame_stride = frame_stride; im.row_stride = row_stride;
    return build_keyframes(h, first, count, img_type, im, sel, K, depth, out);
}

}  // extern "C"
