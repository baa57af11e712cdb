// Inputs that already live in device memory (include/eds_hip_device.h): event frames, event slices, keyframe points and inverse
// depths are read where they are by kernels on the handle's stream.  The host calls (eds_capi_inputs.hip) narrow or pack on the CPU
// into pinned staging that the GPU then reads over PCIe; here the host only checks the pointers and queues.  What a slot holds
// afterwards is what the host call leaves there from the same values, bit for bit: the same narrowing (round-to-nearest-even, fp32
// denormals kept), the same replicated margin, and upload_points' fp64 arithmetic without contraction (this file is compiled with
// -ffp-contract=off, csrc/Makefile).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/eds_hip_device.h"
#include "eds_capi_internal.hpp"

using namespace edscapi;

namespace {

// ---- event frames ------------------------------------------------------------------------------------------------------------------
// Row-major H x W frames of T (float or double) -> the slots' frames (tiles or row-major, padding and the replicated margin
// included), frame blockIdx.z of the call.  A pure layout transform: per frame it reads sizeof(T) H W and writes 4 Hp Wp bytes.
// One workgroup moves a block of 4 allocation rows (one row of tiles) by SF_COLS columns through LDS, because the two sides
// coalesce differently:
//   read   wavefront j takes source row j of the block; a lane reads 16 bytes (4 floats / 2 doubles) at a 16-byte-aligned address
//          whatever the row's own alignment is (pitched sources); the pieces that stick out of the row go element by element
//   write  a lane stores the 16 bytes of one tile row; four lanes one whole 64-byte tile, a wavefront 1 KB of consecutive tiles
//          (row-major frames: a wavefront stores 1 KB of one row)
// The clamp to the frame (= Grid2D's) happens between the two, on LDS indices.
constexpr int SF_COLS = 256, SF_T = 256;
template <class T>
__global__ __launch_bounds__(SF_T) void k_store_frames_dev(const T* __restrict__ src, long long frame_stride, long long row_stride,
                                                         float* __restrict__ frames, int first, int H, int W, int Hp, int Wp, int tiled) {
    constexpr int E = 16 / (int)sizeof(T);              // elements per 16-byte read
    __shared__ float s[4][SF_COLS + 1];
    const int c0 = (int)blockIdx.x * SF_COLS - EDS_FRAME_MARGIN, r0 = (int)blockIdx.y * 4 - EDS_FRAME_MARGIN;     // logical
    // source columns [lo, hi) cover the clamp of every column of the block (a block that lies wholly in the right padding: W - 1 only)
    const int lo = min(max(c0, 0), W - 1), hi = max(min(c0 + SF_COLS, W), lo + 1);
    const T* __restrict__ fr = src + (long long)blockIdx.z * frame_stride;
    {
        const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const T* __restrict__ row = fr + (long long)min(max(r0 + j, 0), H - 1) * row_stride;
        // 16-byte pieces of this row, counted from the aligned address at or below element `lo`
        const int mis = (int)((reinterpret_cast<uintptr_t>(row + lo) / sizeof(T)) & (uintptr_t)(E - 1));
        const int npieces = (mis + (hi - lo) + E - 1) / E;
        for (int k = lane; k < npieces; k += 64) {
            const int e = lo - mis + k * E;             // first element of the piece
            if (e >= lo && e + E <= hi) {
                if (sizeof(T) == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(row + e);
                    s[j][e - lo] = v.x; s[j][e - lo + 1] = v.y; s[j][e - lo + 2] = v.z; s[j][e - lo + 3] = v.w;
                } else {
                    const double2 v = *reinterpret_cast<const double2*>(row + e);
                    s[j][e - lo] = (float)v.x; s[j][e - lo + 1] = (float)v.y;
                }
            } else {
                for (int u = 0; u < E; ++u)
                    if (e + u >= lo && e + u < hi) s[j][e + u - lo] = (float)row[e + u];
            }
        }
    }
    __syncthreads();
    // (tile column, row of the block) of this lane
    const int j = tiled ? (int)(threadIdx.x & 3) : (int)(threadIdx.x >> 6), tc = tiled ? (int)(threadIdx.x >> 2) : (int)(threadIdx.x & 63);
    const int c = c0 + 4 * tc;
    if (c >= Wp - EDS_FRAME_MARGIN) return;
    float4 o;
    o.x = s[j][min(max(c, 0), W - 1) - lo];
    o.y = s[j][min(max(c + 1, 0), W - 1) - lo];
    o.z = s[j][min(max(c + 2, 0), W - 1) - lo];
    o.w = s[j][min(max(c + 3, 0), W - 1) - lo];
    float* __restrict__ dst = frames + (size_t)(first + (int)blockIdx.z) * Hp * Wp;
    *reinterpret_cast<float4*>(dst + eds_frame_index(r0 + j, c, Wp, tiled)) = o;      // c + MARGIN is a multiple of 4: contiguous in either layout
}

// ---- keyframe points ---------------------------------------------------------------------------------------------------------------
// upload_points (eds_capi_inputs.hip) for slots first .. first + gridDim.y - 1, from fp64 device arrays: the eight fp32 planes and the
// cell word.  N and K of a slot come from its pose block, which the caller has just queued in front (fill_static + upload_pose).
// `extent`: the points the host checked the source arrays for (eds_dev_check_range) — no read goes past it, whatever a pose block says.
constexpr int IP_T = 256;
__global__ __launch_bounds__(IP_T) void k_ingest_points(EdsArrays A, int first, long long stride, long long extent, const double* __restrict__ norm_xy,
                                                      const double* __restrict__ grad_xy, const double* __restrict__ idp,
                                                      const double* __restrict__ w) {
    const int i = blockIdx.x * IP_T + threadIdx.x, slot = first + (int)blockIdx.y;
    if (i >= A.Np) return;
    const double* __restrict__ pb = A.pose + (size_t)slot * EDS_POSE_STRIDE;
    const int N = (int)pb[EDS_PB_N];
    const double fx = pb[EDS_PB_K], fy = pb[EDS_PB_K + 1], cx = pb[EDS_PB_K + 2], cy = pb[EDS_PB_K + 3];
    const size_t o = (size_t)slot * A.Np + i;
    const long long p = (long long)blockIdx.y * stride + i;
    const bool in = i < N && p < extent;
    const double x = in ? norm_xy[2 * p] : 0.0, y = in ? norm_xy[2 * p + 1] : 0.0;
    const_cast<float*>(A.x)[o] = (float)x;
    const_cast<float*>(A.y)[o] = (float)y;
    const_cast<float*>(A.rho)[o] = in ? (float)idp[p] : 1.f;
    const_cast<float*>(A.gx)[o] = in ? (float)grad_xy[2 * p] : 0.f;
    const_cast<float*>(A.gy)[o] = in ? (float)grad_xy[2 * p + 1] : 0.f;
    const_cast<float*>(A.w)[o] = in ? (float)w[p] : 0.f;
    // the point's own keyframe pixel in fp64, split into an integer cell and an fp32 fraction (as upload_points: no contraction)
    const double u0 = in ? fx * x + cx : 0.0, v0 = in ? fy * y + cy : 0.0;
    double cu = floor(u0), cv = floor(v0);
    if (!(cu > -32000.0)) cu = -32000.0; if (cu > 32000.0) cu = 32000.0;
    if (!(cv > -32000.0)) cv = -32000.0; if (cv > 32000.0) cv = 32000.0;
    const_cast<float*>(A.f0x)[o] = (float)(u0 - cu);
    const_cast<float*>(A.f0y)[o] = (float)(v0 - cv);
    const_cast<int*>(A.cell0)[o] = (int)(((unsigned)(int)cv << 16) | ((unsigned)(int)cu & 0xffffu));
}

// the rho plane alone (eds_trk_set_idepth_strided's narrowing and padding); N from the pose block; extent (doubles) as above
__global__ __launch_bounds__(IP_T) void k_ingest_idepths(EdsArrays A, int first, long long stride, int elem_stride, long long extent,
                                                       const double* __restrict__ idp) {
    const int i = blockIdx.x * IP_T + threadIdx.x, slot = first + (int)blockIdx.y;
    if (i >= A.Np) return;
    const int N = (int)A.pose[(size_t)slot * EDS_POSE_STRIDE + EDS_PB_N];
    const long long e = ((long long)blockIdx.y * stride + i) * elem_stride;
    const_cast<float*>(A.rho)[(size_t)slot * A.Np + i] = i < N && e < extent ? (float)idp[e] : 1.f;
}

const char* memory_type_name(hipMemoryType t) {
    switch (t) {
        case hipMemoryTypeHost: return "pinned host memory";
        case hipMemoryTypeDevice: return "device memory";
        case hipMemoryTypeArray: return "a HIP array";
        case hipMemoryTypeUnified: return "unified memory";
        case hipMemoryTypeManaged: return "managed memory";
        default: return "memory the HIP runtime does not know (pageable host memory?)";
    }
}

std::string hex(const void* p) {
    char b[32];
    std::snprintf(b, sizeof(b), "%p", p);
    return b;
}

int check_named(int device, const void* p, size_t bytes, const char* what) {
    const std::string who = std::string(what) + " " + hex(p) + ": ";
    if (!p) return fail(EDS_ERR_INVALID, std::string(what) + ": NULL pointer");
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(EDS_ERR_INVALID, who + "not known to the HIP runtime (pageable host memory?): " + hipGetErrorString(e));
    }
    if (at.type == hipMemoryTypeDevice) {
        if (at.device != device)
            return fail(EDS_ERR_INVALID, who + "memory of device " + std::to_string(at.device) + ", the kernels run on device " + std::to_string(device));
    } else if (at.type == hipMemoryTypeHost) {
        if (!at.devicePointer || at.devicePointer != p)
            return fail(EDS_ERR_INVALID, who + "pinned host memory that is not mapped into the device at this address");
    } else {
        return fail(EDS_ERR_INVALID, who + memory_type_name(at.type) + ", neither device memory nor mapped pinned host memory");
    }
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, const_cast<void*>(p)) != hipSuccess || !base) {
        (void)hipGetLastError();
        return fail(EDS_ERR_INVALID, who + memory_type_name(at.type) + " whose allocation the HIP runtime cannot report");
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b0 = reinterpret_cast<uintptr_t>(base);
    if (a < b0 || a - b0 > size || bytes > size - (a - b0))
        return fail(EDS_ERR_INVALID, who + std::to_string(bytes) + " bytes run past its allocation (" + memory_type_name(at.type) + ", " +
                                         std::to_string(size) + " bytes from " + hex(base) + ")");
    return EDS_OK;
}

// the checks every ingest call starts with, in this order: handle and slot range, then "no batch in flight"
int check_call(eds_trk* h, int first, int count) {
    const int rc = check_range(h, first, count);
    return rc ? rc : check_idle_slots(h, first, count, 0);
}

}  // namespace

extern "C" {

int eds_dev_abi_version(void) { return EDS_HIP_DEVICE_ABI_VERSION; }

int eds_dev_check_range(int device, const void* p, size_t bytes) { return check_named(device, p, bytes, "pointer"); }

int eds_dev_malloc(int device, size_t bytes, void** d_ptr) {
    if (!d_ptr) return fail(EDS_ERR_INVALID, "null output");
    *d_ptr = nullptr;
    if (bytes == 0) return fail(EDS_ERR_INVALID, "zero bytes");
    EDS_HIP_TRY(hipSetDevice(device));
    EDS_HIP_TRY(hipMalloc(d_ptr, bytes));
    return EDS_OK;
}

int eds_dev_free(void* d_ptr) {
    if (!d_ptr) return EDS_OK;
    EDS_HIP_TRY(hipFree(d_ptr));
    return EDS_OK;
}

int eds_dev_upload(void* d_dst, const void* h_src, size_t bytes) {
    if (!d_dst || !h_src) return fail(EDS_ERR_INVALID, "null argument");
    if (bytes) EDS_HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return EDS_OK;
}

int eds_dev_download(void* h_dst, const void* d_src, size_t bytes) {
    if (!h_dst || !d_src) return fail(EDS_ERR_INVALID, "null argument");
    if (bytes) EDS_HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return EDS_OK;
}

int eds_dev_wait_stream(eds_trk* h, void* producer_stream) {
    if (!h) return fail(EDS_ERR_INVALID, "null handle");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (!h->ev_dev_in) EDS_HIP_TRY(hipEventCreateWithFlags(&h->ev_dev_in, hipEventDisableTiming));
    EDS_HIP_TRY(hipEventRecord(h->ev_dev_in, static_cast<hipStream_t>(producer_stream)));
    EDS_HIP_TRY(hipStreamWaitEvent(h->own.st, h->ev_dev_in, 0));
    return EDS_OK;
}

int eds_dev_signal_stream(eds_trk* h, void* consumer_stream) {
    if (!h) return fail(EDS_ERR_INVALID, "null handle");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if (!h->ev_dev_out) EDS_HIP_TRY(hipEventCreateWithFlags(&h->ev_dev_out, hipEventDisableTiming));
    EDS_HIP_TRY(hipEventRecord(h->ev_dev_out, h->own.st));
    EDS_HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), h->ev_dev_out, 0));
    return EDS_OK;
}

int eds_dev_set_event_frames(eds_trk* h, int first, int count, int dtype, const void* d_frames, int64_t frame_stride, int64_t row_stride) {
    int rc = check_call(h, first, count);
    if (rc) return rc;
    if (dtype != EDS_IMG_F32 && dtype != EDS_IMG_F64) return fail(EDS_ERR_INVALID, "dtype must be EDS_IMG_F32 or EDS_IMG_F64");
    const int64_t H = h->H, W = h->W;
    if (row_stride == 0) row_stride = W;
    if (frame_stride == 0) frame_stride = (H - 1) * row_stride + W;
    if (row_stride < W || frame_stride < (H - 1) * row_stride + W || frame_stride > (int64_t)1 << 40)
        return fail(EDS_ERR_INVALID, "bad strides: row_stride >= W and frame_stride >= (H - 1) * row_stride + W, in elements (0 = dense)");
    const size_t esz = dtype == EDS_IMG_F32 ? 4 : 8;
    if (d_frames && (reinterpret_cast<uintptr_t>(d_frames) & (esz - 1))) return fail(EDS_ERR_INVALID, "d_frames is not aligned to its element size");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = check_named(h->own.dev, d_frames, (size_t)((count - 1) * frame_stride + (H - 1) * row_stride + W) * esz, "d_frames"))) return rc;
    if ((rc = unshare_frames(h, first, count))) return rc;
    const dim3 grid((h->Wp + SF_COLS - 1) / SF_COLS, h->Hp / 4, count);
    float* frames = h->dframe;
    if (dtype == EDS_IMG_F32)
        hipLaunchKernelGGL(k_store_frames_dev<float>, grid, dim3(SF_T), 0, h->own.st, static_cast<const float*>(d_frames), (long long)frame_stride,
                           (long long)row_stride, frames, first, h->H, h->W, h->Hp, h->Wp, h->tiled);
    else
        hipLaunchKernelGGL(k_store_frames_dev<double>, grid, dim3(SF_T), 0, h->own.st, static_cast<const double*>(d_frames), (long long)frame_stride,
                           (long long)row_stride, frames, first, h->H, h->W, h->Hp, h->Wp, h->tiled);
    const hipError_t e = hipGetLastError();
    // after a failed launch the slots no longer count as holding a frame (include/eds_hip_device.h), and their strip copies are stale
    for (int s = first; s < first + count; ++s) { h->slots[s].has_frame = e == hipSuccess; ++h->slots[s].frame_version; }
    if (e != hipSuccess) return fail(EDS_ERR_HIP, hipGetErrorString(e));
    return EDS_OK;
}

int eds_dev_build_event_frames(eds_trk* h, int first_slot, int count, const int* offsets, const uint16_t* d_x, const uint16_t* d_y,
                               const uint8_t* d_polarity, int level, double blur_sigma, int use_exp_weights, double* norms) {
    int rc = check_call(h, first_slot, count);
    if (rc) return rc;
    if (!offsets || offsets[0] < 0) return fail(EDS_ERR_INVALID, "bad offsets");
    for (int b = 0; b < count; ++b) if (offsets[b + 1] < offsets[b]) return fail(EDS_ERR_INVALID, "offsets must not decrease");
    if (level < 0 || level > 16) return fail(EDS_ERR_INVALID, "bad level");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t e0 = (size_t)offsets[0], ne = (size_t)offsets[count] - e0;
    if (ne > 0) {
        if (reinterpret_cast<uintptr_t>(d_x) & 1 || reinterpret_cast<uintptr_t>(d_y) & 1) return fail(EDS_ERR_INVALID, "d_x / d_y are not aligned to uint16");
        if ((rc = check_named(h->own.dev, d_x ? d_x + e0 : nullptr, ne * 2, "d_x"))) return rc;
        if ((rc = check_named(h->own.dev, d_y ? d_y + e0 : nullptr, ne * 2, "d_y"))) return rc;
        if ((rc = check_named(h->own.dev, d_polarity ? d_polarity + e0 : nullptr, ne, "d_polarity"))) return rc;
    }
    if ((rc = unshare_frames(h, first_slot, count))) return rc;
    return eds_frame_build_batch(h, first_slot, count, offsets, d_x, d_y, d_polarity, level, blur_sigma, use_exp_weights, norms, true);
}

int eds_dev_set_keyframes(eds_trk* h, int first, int count, const int* N, const double* d_norm_xy, const double* d_grad_xy,
                          const double* d_idp, const double* d_w, int64_t stride, const double* K) {
    int rc = check_call(h, first, count);
    if (rc) return rc;
    if (!N || !K) return fail(EDS_ERR_INVALID, "null N or K");
    int64_t maxN = 0, extent = 0;                        // points from the arrays' start to the end of the last one read
    for (int b = 0; b < count; ++b) {
        if (N[b] < 1 || N[b] > h->Nmax) return fail(EDS_ERR_INVALID, "N out of range for this handle");
        maxN = std::max<int64_t>(maxN, N[b]);
    }
    if (stride < maxN || stride > (int64_t)1 << 40) return fail(EDS_ERR_INVALID, "stride must be at least the largest N");
    for (int b = 0; b < count; ++b) extent = std::max<int64_t>(extent, b * stride + N[b]);
    const double* arrs[4] = {d_norm_xy, d_grad_xy, d_idp, d_w};
    for (const double* a : arrs) if (reinterpret_cast<uintptr_t>(a) & 7) return fail(EDS_ERR_INVALID, "a keyframe array is not aligned to a double");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = check_named(h->own.dev, d_norm_xy, (size_t)extent * 16, "d_norm_xy"))) return rc;
    if ((rc = check_named(h->own.dev, d_grad_xy, (size_t)extent * 16, "d_grad_xy"))) return rc;
    if ((rc = check_named(h->own.dev, d_idp, (size_t)extent * 8, "d_idp"))) return rc;
    if ((rc = check_named(h->own.dev, d_w, (size_t)extent * 8, "d_w"))) return rc;
    for (int b = 0; b < count; ++b) {                   // N and K reach the kernels through the slots' pose blocks
        Slot& s = h->slots[first + b];
        s.N = N[b];
        s.num_points = N[b];
        for (int k = 0; k < 4; ++k) s.K[k] = K[4 * b + k];
        fill_static(h, first + b);
    }
    // from here on a failure is a HIP failure with work possibly queued: the planes of the range may be half-written, so its slots no
    // longer count as holding a keyframe (include/eds_hip_device.h) — the same rule as a failed eds_trk_set_event_frames for has_frame
    hipError_t e = hipSuccess;
    if ((rc = upload_pose(h, first, count)) == EDS_OK) {
        hipLaunchKernelGGL(k_ingest_points, dim3(h->Np / IP_T, count), dim3(IP_T), 0, h->own.st, h->arrays(), first, (long long)stride, (long long)extent,
                           d_norm_xy, d_grad_xy, d_idp, d_w);
        e = hipGetLastError();
        if (e == hipSuccess) {
            eds_launch_gram_batch(h->arrays(), first, count, effective_blocks(h), h->own.st);
            e = hipGetLastError();
        }
        if (e != hipSuccess) rc = fail(EDS_ERR_HIP, hipGetErrorString(e));
    }
    if (rc) {
        for (int sl = first; sl < first + count; ++sl) { h->slots[sl].has_kf = false; h->slots[sl].seeded = false; h->slots[sl].epi_valid = false; }
        return rc;
    }
    for (int sl = first; sl < first + count; ++sl) {    // as eds_trk_set_keyframe
        Slot& s = h->slots[sl];
        s.gram_host_stale = true;                       // the Gram matrices are in HBM only: fill_pose fetches them for a host-side reader
        s.has_kf = true;
        s.seeded = false;
        eds_klt_reset_slot(h, sl);
        s.epi_valid = false;
        s.residuals.clear();
        s.res_on_device = false; s.trace_on_device = false; s.ntrace = 0;
    }
    return EDS_OK;
}

int eds_dev_set_idepths(eds_trk* h, int first, int count, const double* d_idp, int64_t stride, int elem_stride) {
    int rc = check_call(h, first, count);
    if (rc) return rc;
    if (elem_stride < 1) return fail(EDS_ERR_INVALID, "elem_stride must be at least 1");
    int64_t maxN = 0, extent = 0;
    for (int s = first; s < first + count; ++s) {
        if (!h->slots[s].has_kf) return fail(EDS_ERR_STATE, "keyframe not set");
        maxN = std::max<int64_t>(maxN, h->slots[s].N);
    }
    if (stride < maxN || stride > (int64_t)1 << 40) return fail(EDS_ERR_INVALID, "stride must be at least the largest N of the range");
    for (int b = 0; b < count; ++b) extent = std::max<int64_t>(extent, (b * stride + h->slots[first + b].N - 1) * elem_stride + 1);
    if (reinterpret_cast<uintptr_t>(d_idp) & 7) return fail(EDS_ERR_INVALID, "d_idp is not aligned to a double");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    if ((rc = check_named(h->own.dev, d_idp, (size_t)extent * 8, "d_idp"))) return rc;
    // (the pose blocks in HBM hold the slots' N already: eds_trk_set_idepth's one-launch path relies on the same)
    hipLaunchKernelGGL(k_ingest_idepths, dim3(h->Np / IP_T, count), dim3(IP_T), 0, h->own.st, h->arrays(), first, (long long)stride, elem_stride, (long long)extent, d_idp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        eds_launch_gram_batch(h->arrays(), first, count, effective_blocks(h), h->own.st);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {              // rho planes and Gram matrices may disagree: the slots need their keyframe again
        for (int s = first; s < first + count; ++s) h->slots[s].has_kf = false;
        return fail(EDS_ERR_HIP, hipGetErrorString(e));
    }
    for (int s = first; s < first + count; ++s) h->slots[s].gram_host_stale = true;
    return EDS_OK;
}

}  // extern "C"
