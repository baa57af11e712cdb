// Keyframe point set-up on the device for gfx950.
//
// What the reference does once per keyframe on the CPU with OpenCV (KeyFrame::create, KeyFrame.cpp:333-463):
//   image -> [0,1] -> log(img + 0.2)                          :363-374
//   Sobel 3x3 in x and y, gradient magnitude                  :384-401
//   candidatePoints: 20x20 cells; MAX = k strongest per cell, MEDIAN = everything above the cell median   :740-823
//   norm_coord = (coord - c)/f, grad = Sobel at the pixel     :413-430
//   setDepthMap: nearest depth-map point -> idp, distance -> weight in [0,1]     :1137-1198
//   cleanPoints(0.7): drop weight < 0.7, order preserved      :1566-1587
// Here: all of it in fp64 on the GPU, ending directly in the slot's SoA planes (no N x 6 upload), with the
// index-aligned fp64 arrays kept for the caller's KeyFrame container (eds_trk_get_keyframe_points).
//
// Bandwidth-shaped, integer/selection work — no MFMA.  Selection per cell is rank-by-counting in LDS (a 400-element
// cell needs 160 k comparisons; 768 cells per VGA image), which reproduces cv::minMaxLoc's first-in-row-major tie
// rule and std::nth_element's order statistic without sorting.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "eds_handle.hpp"
#include "eds_kdtree.hpp"

#pragma clang fp contract(off)      // sums are formed exactly as written (the oracle states the same association)

#include "eds_keyframe_kernels.hpp"

static int ensure(eds_trk* h) {
    EdsKeyframeBuffers& kb = h->kf_build;
    if (kb.d_raw) return EDS_OK;
    const size_t n = (size_t)h->H * h->W;
    if (!h->own.alloc({{&kb.d_raw, n * 8}, {(void**)&kb.d_log, n * 8}, {(void**)&kb.d_gx, n * 8}, {(void**)&kb.d_gy, n * 8}, {(void**)&kb.d_mag, n * 8},
                       {(void**)&kb.d_idp, n * 8}, {(void**)&kb.d_w, n * 8}, {(void**)&kb.d_coord, n * 16}, {(void**)&kb.d_grad, n * 16},
                       {(void**)&kb.d_partial, 2 * 256 * 8}, {(void**)&kb.d_cand, n * 4}, {(void**)&kb.d_cnt, (n / 4 + 2) * 4},       // cells are at least 2 x 2
                       {(void**)&kb.d_off, (n / 4 + 2) * 4}, {(void**)&kb.d_summary, 16}}))
        return eds_internal_fail(EDS_ERR_HIP, "hipMalloc (keyframe set-up buffers)");
    return EDS_OK;
}

int eds_keyframe_build(eds_trk* h, int slot, int img_type, const void* img, int img_H, int img_W, int channels, const eds_kf_select* sel,
                       int n_depth, const double* depth_xy, const double* depth_idp, double fx, double fy, double cx, double cy, int* n_points) {
    const int H = h->H, W = h->W;
    const size_t n = (size_t)H * W;
    if (img_H <= 0 || img_W <= 0) { img_H = H; img_W = W; }
    if (channels != 1 && channels != 3) return eds_internal_fail(EDS_ERR_INVALID, "an image has 1 (grey) or 3 (RGB, interleaved) channels");
    if (channels == 3 && img_type == 2) return eds_internal_fail(EDS_ERR_INVALID, "cv::cvtColor takes 8-bit or float colour images, not CV_64F");
    if (img_H < 2 || img_W < 2) return eds_internal_fail(EDS_ERR_INVALID, "bad image size");
    const bool prepare = channels != 1 || img_H != H || img_W != W;
    const int cell = sel->cell;
    if (cell < 2 || cell > KF_MAX_CELL || cell > H || cell > W) return eds_internal_fail(EDS_ERR_INVALID, "cell size must be in [2, 32] and fit the image");
    if (sel->method != EDS_KF_MAX && sel->method != EDS_KF_MEDIAN) return eds_internal_fail(EDS_ERR_INVALID, "unknown point selection method");
    if (img_type < 0 || img_type > 2) return eds_internal_fail(EDS_ERR_INVALID, "img_type must be EDS_IMG_U8, EDS_IMG_F32 or EDS_IMG_F64");
    if (n_depth > 0 && (!depth_xy || !depth_idp)) return eds_internal_fail(EDS_ERR_INVALID, "null depth map");
    int rc = ensure(h);
    if (rc) return rc;
    EdsKeyframeBuffers& kb = h->kf_build;
    kb.last_slot = -1;
    if (n_depth > kb.cap_depth) {
        const int want = n_depth + n_depth / 4 + 256;
        if (!h->own.regrow(kb.cap_depth, want, {{(void**)&kb.d_dxy, (size_t)want * 16}, {(void**)&kb.d_didp, (size_t)want * 8}}))
            return eds_internal_fail(EDS_ERR_HIP, "hipMalloc (depth map)");
    }
    hipStream_t st = h->own.st;
    const size_t px = img_type == 0 ? 1 : (img_type == 1 ? 4 : 8);
    hipError_t e = hipSuccess;
    if (!prepare) {
        e = hipMemcpyAsync(kb.d_raw, img, n * px, hipMemcpyHostToDevice, st);
    } else {                            // resize and / or grey conversion on the device (KeyFrame.cpp:352-362), into the usual buffer
        const size_t src_bytes = (size_t)img_H * img_W * channels * px;
        if (src_bytes > kb.src_bytes && !h->own.regrow(kb.src_bytes, src_bytes, {{&kb.d_src, src_bytes}}))
            return eds_internal_fail(EDS_ERR_HIP, "hipMalloc (source image)");
        e = hipMemcpyAsync(kb.d_src, img, src_bytes, hipMemcpyHostToDevice, st);
        const dim3 g((W + KF_T - 1) / KF_T, H), b(KF_T);
        if (img_type == 0) hipLaunchKernelGGL(k_prepare<uint8_t>, g, b, 0, st, (const uint8_t*)kb.d_src, img_H, img_W, channels, (uint8_t*)kb.d_raw, H, W);
        else if (img_type == 1) hipLaunchKernelGGL(k_prepare<float>, g, b, 0, st, (const float*)kb.d_src, img_H, img_W, channels, (float*)kb.d_raw, H, W);
        else hipLaunchKernelGGL(k_prepare<double>, g, b, 0, st, (const double*)kb.d_src, img_H, img_W, channels, (double*)kb.d_raw, H, W);
    }
    if (e != hipSuccess) return eds_internal_fail(EDS_ERR_HIP, hipGetErrorString(e));
    const int NB = 256;
    hipLaunchKernelGGL(k_minmax, dim3(NB), dim3(KF_T), 0, st, kb.d_raw, img_type, n, kb.d_partial);
    hipLaunchKernelGGL(k_log, dim3(NB), dim3(KF_T), 0, st, kb.d_raw, img_type, n, kb.d_partial, NB, kb.d_log);
    if (sel->sobel_ksize == 7) hipLaunchKernelGGL(k_sobel7, dim3((W + KF_T - 1) / KF_T, H), dim3(KF_T), 0, st, kb.d_log, H, W, kb.d_gx, kb.d_gy, kb.d_mag);
    else hipLaunchKernelGGL(k_sobel, dim3((W + KF_T - 1) / KF_T, H), dim3(KF_T), 0, st, kb.d_log, H, W, kb.d_gx, kb.d_gy, kb.d_mag);
    const int ncx = W / cell, ncy = H / cell, ncell = ncx * ncy;       // only whole cells (KeyFrame.cpp:752-754)
    const int k_per_cell = sel->method == EDS_KF_MAX ? (sel->num_points > 0 ? sel->num_points / ncell : 0) : 0;
    hipLaunchKernelGGL(k_select, dim3(ncell), dim3(KF_T), 0, st, kb.d_mag, W, cell, ncx, (int)sel->method, k_per_cell, kb.d_cand, kb.d_cnt);
    hipLaunchKernelGGL(k_scan_cells, dim3(1), dim3(KF_T), 0, st, kb.d_cnt, ncell, kb.d_off);
    hipLaunchKernelGGL(k_emit, dim3(ncell), dim3(KF_T), 0, st, kb.d_cand, kb.d_cnt, kb.d_off, cell, ncx, W, kb.d_gx, kb.d_gy, kb.d_coord, kb.d_grad);
    // the depth map's k-d tree, built on the host while the device works on the image; uploaded in tree order
    if (n_depth > 0) {
        kb.h_perm.resize(n_depth); kb.h_txy.resize(2 * (size_t)n_depth); kb.h_tidp.resize(n_depth);
        edskd::build_tree(depth_xy, n_depth, kb.h_perm.data());
        for (int k = 0; k < n_depth; ++k) {
            const int j = kb.h_perm[k];
            kb.h_txy[2 * (size_t)k] = depth_xy[2 * (size_t)j]; kb.h_txy[2 * (size_t)k + 1] = depth_xy[2 * (size_t)j + 1];
            kb.h_tidp[k] = depth_idp[j];
        }
        e = hipMemcpyAsync(kb.d_dxy, kb.h_txy.data(), (size_t)n_depth * 16, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(kb.d_didp, kb.h_tidp.data(), (size_t)n_depth * 8, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return eds_internal_fail(EDS_ERR_HIP, hipGetErrorString(e));
    }
    int ncand = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&ncand, kb.d_off + ncell, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return eds_internal_fail(EDS_ERR_HIP, hipGetErrorString(e));
    if (ncand < 1) return eds_internal_fail(EDS_ERR_INVALID, "the selection produced no candidate point");
    const double const_idp = 1.0 / ((sel->max_depth - sel->min_depth) / 2.0);       // KeyFrame.cpp:1189
    if (n_depth > 0) {
        hipLaunchKernelGGL(k_nearest_tree, dim3((ncand + KF_T - 1) / KF_T), dim3(KF_T), 0, st, kb.d_coord, ncand, kb.d_dxy, kb.d_didp, n_depth,
                           kb.d_idp, kb.d_w);
        hipLaunchKernelGGL(k_minmax, dim3(NB), dim3(KF_T), 0, st, (const void*)kb.d_w, 2, (size_t)ncand, kb.d_partial);
    }
    hipLaunchKernelGGL(k_weights_clean, dim3(1), dim3(1024), 0, st, kb.d_coord, kb.d_grad, kb.d_idp, kb.d_w, ncand, n_depth > 0 ? 1 : 0,
                       const_idp, kb.d_partial, NB, sel->weight_threshold, kb.d_summary);
    int summary[2] = {0, 0};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(summary, kb.d_summary, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return eds_internal_fail(EDS_ERR_HIP, hipGetErrorString(e));
    const int N = summary[1];
    if (n_points) *n_points = N;
    kb.last_N = N; kb.last_candidates = ncand;
    kb.K[0] = fx; kb.K[1] = fy; kb.K[2] = cx; kb.K[3] = cy;
    if (N < 1) return eds_internal_fail(EDS_ERR_INVALID, "no point survived the weight threshold");
    if (N > h->Nmax) return eds_internal_fail(EDS_ERR_INVALID, "the keyframe has more points than the handle's max_points");
    hipLaunchKernelGGL(k_fill_slot, dim3(h->Np / KF_T), dim3(KF_T), 0, st, h->arrays(), slot, N, fx, fy, cx, cy, kb.d_coord, kb.d_grad, kb.d_idp, kb.d_w);
    e = hipGetLastError();
    if (e != hipSuccess) return eds_internal_fail(EDS_ERR_HIP, hipGetErrorString(e));
    Slot& s = h->slots[slot];
    s.N = N; s.K[0] = fx; s.K[1] = fy; s.K[2] = cx; s.K[3] = cy;
    s.num_points = ncand;                   // candidatePoints assigns it (KeyFrame.cpp:820); cleanPoints does not touch it
    if ((rc = eds_internal_refresh_gram(h, slot))) return rc;
    s.has_kf = true;
    s.seeded = false;                       // as eds_trk_set_keyframe
    eds_klt_reset_slot(h, slot);
    s.epi_valid = false;
    s.residuals.clear();
    s.res_on_device = false; s.trace_on_device = false; s.ntrace = 0;     // as eds_trk_set_keyframe
    kb.last_slot = slot;
    return EDS_OK;
}

int eds_keyframe_get_points(eds_trk* h, int slot, double* coord_xy, double* norm_xy, double* grad_xy, double* idp, double* weights) {
    EdsKeyframeBuffers& kb = h->kf_build;
    if (kb.last_slot != slot || kb.last_N < 1) return eds_internal_fail(EDS_ERR_STATE, "this slot is not the one eds_trk_build_keyframe filled last");
    const size_t N = (size_t)kb.last_N;
    hipError_t e = hipStreamSynchronize(h->own.st);
    if (e == hipSuccess && (coord_xy || norm_xy)) {
        double* dst = coord_xy ? coord_xy : norm_xy;
        e = hipMemcpy(dst, kb.d_coord, N * 16, hipMemcpyDeviceToHost);
        if (e == hipSuccess && norm_xy) {
            for (size_t i = 0; i < N; ++i) {                      // KeyFrame.cpp:417-423
                const double x = dst[2 * i], y = dst[2 * i + 1];
                norm_xy[2 * i] = (x - kb.K[2]) / kb.K[0];
                norm_xy[2 * i + 1] = (y - kb.K[3]) / kb.K[1];
            }
        }
    }
    if (e == hipSuccess && grad_xy) e = hipMemcpy(grad_xy, kb.d_grad, N * 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess && idp) e = hipMemcpy(idp, kb.d_idp, N * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && weights) e = hipMemcpy(weights, kb.d_w, N * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return eds_internal_fail(EDS_ERR_HIP, hipGetErrorString(e));
    return EDS_OK;
}
