// include/eds_hip_undistort.h: raw uint8 / uint16 frames to rectified, photometrically corrected fp32 planes on the device.  The set-up
// (K, the map, G, the inverse vignette) is the host code of eds_undistort.hpp, run here once per camera and uploaded; per frame the
// kernels below do table reads, fp32 products and sums through the same header's corrected() and bilinear().  Built without
// contraction into FMAs (csrc/Makefile).
//
// One workgroup is 64 x 4 output pixels: a wavefront stores 64 consecutive floats of one row (256 bytes, full width), and the four
// rows of a workgroup share most of the raw rows their taps gather from.  blockIdx.z is the frame, so processFrame's per-frame branch
// is uniform in a workgroup.
//   k_und_fused     one launch per call over count x h x w: the map pair, the four raw taps, each corrected on the fly (a tap's value is
//                   one fp32 product of two table reads, so this is the two-pass result bit for bit), the bilinear sum.  For uint8 the
//                   256 entries of G a frame can index are staged in LDS (1 KB); the 65 536 entries a uint16 frame indexes (256 KB) do
//                   not fit a CU's 160 KB and are read from global memory.
//   k_und_plane     processFrame<T> alone over count x h_org x w_org: the first of the two passes, and all of a passthrough handle.
//   k_und_remap     the second pass, from the fp32 plane.
// eds_und_set_form pins k_und_fused or k_und_plane + k_und_remap; left alone, the size of the call chooses (AUTO_TWO_PASS_PIXELS below);
// tools/bench_undistort.py measures all three.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eds_hip_undistort.h"
#include "eds_device_owner.hpp"
#include "eds_undistort.hpp"

using edscapi::fail;
using edscapi::read_back;

static_assert(sizeof(edsund::Geometry) == sizeof(eds_und_geometry), "edsund::Geometry is eds_und_geometry member for member");
static_assert(offsetof(edsund::Geometry, out_pars) == offsetof(eds_und_geometry, out_pars), "edsund::Geometry is eds_und_geometry member for member");
static_assert(sizeof(edsund::Settings) == sizeof(eds_und_settings), "edsund::Settings is eds_und_settings member for member");
static_assert(edsund::MAX_SLOTS == EDS_UND_MAX_SLOTS && edsund::MAX_SLOTS <= 32, "one bit per frame in Frames::phot_mask");
static_assert(edsund::MODEL_PINHOLE == EDS_UND_MODEL_PINHOLE && edsund::OUT_FULL == EDS_UND_OUT_FULL && edsund::RAW_U16 == EDS_UND_U16, "header constants");

struct eds_und {
    edscapi::DeviceOwner own;
    edsund::Setup s;
    edsund::Photometric ph;
    edsund::Settings st = edsund::settings_default();
    int slots = 0;
    int form = EDS_UND_FORM_AUTO;
    bool passthrough = false;       // s.passthrough until eds_und_set_map
    float2* d_map = nullptr;        // {remapX, remapY} per output pixel
    float* d_planes = nullptr;      // slots x h x w
    float* d_G = nullptr;           // MAX_G_DEPTH floats
    float* d_vinv = nullptr;        // h_org x w_org
    void* d_raw = nullptr;          // host frames staged dense; grows with the largest call
    size_t raw_bytes = 0;
    float* d_phot = nullptr;        // the two-pass form's photometric planes; grows likewise
    size_t phot_bytes = 0;
};

namespace {

constexpr int TX = 64, TY = 4;
// EDS_UND_FORM_AUTO: measured on MI355X (profiles/undistort_timing.json), the fused kernel is the faster form at 0.3 M and 1.3 M raw
// pixels a call, the two forms are within 3 % at 4.9 M and the two-pass form is 23 % faster at 21 M
constexpr int64_t AUTO_TWO_PASS_PIXELS = (int64_t)4 << 20;

struct Frames {
    const void* raw;                // frame 0; elements of T
    int64_t rs, fs;                 // in elements
    uint32_t phot_mask;             // bit k: frame k takes processFrame's photometric branch
    int vig;                        // setting_photometricCalibration == 2
    float factor;
    const float* G;
    const float* vinv;
    int w_org, h_org, w, h;
};

template <class T, bool LDS_G>
__global__ void __launch_bounds__(TX* TY) k_und_fused(Frames a, const float2* __restrict__ map, float* __restrict__ planes) {
    __shared__ float sG[LDS_G ? 256 : 1];
    const int f = blockIdx.z;
    const bool phot = (a.phot_mask >> f) & 1u;
    if (LDS_G && phot) sG[threadIdx.y * TX + threadIdx.x] = a.G[threadIdx.y * TX + threadIdx.x];
    __syncthreads();
    const int x = blockIdx.x * TX + threadIdx.x, y = blockIdx.y * TY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const int64_t idx = (int64_t)y * a.w + x;
    const float2 m = map[idx];
    float v = 0.0f;
    if (!edsund::outside(m.x)) {
        float xx = m.x, yy = m.y;
        const int xxi = (int)xx, yyi = (int)yy;         // 0 .. w_org - 2 and 0 .. h_org - 2: every stored pair is map_pair_valid
        xx -= (float)xxi;
        yy -= (float)yyi;
        const T* src = static_cast<const T*>(a.raw) + (int64_t)f * a.fs + (int64_t)yyi * a.rs + xxi;
        const int64_t i = (int64_t)yyi * a.w_org + xxi;
        const float* G = LDS_G ? sG : a.G;
        const float s0 = edsund::corrected((int)src[0], phot, a.vig, G, a.vinv, i, a.factor);
        const float s1 = edsund::corrected((int)src[1], phot, a.vig, G, a.vinv, i + 1, a.factor);
        const float sw = edsund::corrected((int)src[a.rs], phot, a.vig, G, a.vinv, i + a.w_org, a.factor);
        const float sw1 = edsund::corrected((int)src[a.rs + 1], phot, a.vig, G, a.vinv, i + a.w_org + 1, a.factor);
        v = edsund::bilinear(xx, yy, s0, s1, sw, sw1);
    }
    planes[(int64_t)f * a.w * a.h + idx] = v;
}

template <class T, bool LDS_G>
__global__ void __launch_bounds__(TX* TY) k_und_plane(Frames a, float* __restrict__ planes) {
    __shared__ float sG[LDS_G ? 256 : 1];
    const int f = blockIdx.z;
    const bool phot = (a.phot_mask >> f) & 1u;
    if (LDS_G && phot) sG[threadIdx.y * TX + threadIdx.x] = a.G[threadIdx.y * TX + threadIdx.x];
    __syncthreads();
    const int x = blockIdx.x * TX + threadIdx.x, y = blockIdx.y * TY + threadIdx.y;
    if (x >= a.w_org || y >= a.h_org) return;
    const int64_t i = (int64_t)y * a.w_org + x;
    const T* src = static_cast<const T*>(a.raw) + (int64_t)f * a.fs + (int64_t)y * a.rs + x;
    planes[(int64_t)f * a.w_org * a.h_org + i] = edsund::corrected((int)src[0], phot, a.vig, LDS_G ? sG : a.G, a.vinv, i, a.factor);
}

__global__ void __launch_bounds__(TX* TY) k_und_remap(const float* __restrict__ phot_planes, const float2* __restrict__ map, float* __restrict__ planes,
                                                      int w_org, int h_org, int w, int h) {
    const int f = blockIdx.z;
    const int x = blockIdx.x * TX + threadIdx.x, y = blockIdx.y * TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int64_t idx = (int64_t)y * w + x;
    const float2 m = map[idx];
    float v = 0.0f;
    if (!edsund::outside(m.x)) {
        float xx = m.x, yy = m.y;
        const int xxi = (int)xx, yyi = (int)yy;
        xx -= (float)xxi;
        yy -= (float)yyi;
        const float* src = phot_planes + (int64_t)f * w_org * h_org + (int64_t)yyi * w_org + xxi;
        v = edsund::bilinear(xx, yy, src[0], src[1], src[w_org], src[1 + w_org]);
    }
    planes[(int64_t)f * w * h + idx] = v;
}

dim3 grid_of(int w, int h, int count) { return dim3((unsigned)((w + TX - 1) / TX), (unsigned)((h + TY - 1) / TY), (unsigned)count); }

int upload_map(eds_und* h, const float* mapx, const float* mapy) {
    const size_t n = (size_t)h->s.g.w * h->s.g.h;
    std::vector<float2> m(n);
    for (size_t i = 0; i < n; ++i) m[i] = make_float2(mapx[i], mapy[i]);
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_map, m.data(), n * sizeof(float2), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

int upload_G(eds_und* h) {
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_G, h->ph.G.data(), (size_t)h->ph.g_depth * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    return EDS_OK;
}

// a buffer that only grows; false when the device refuses (the old one is gone then, and its size is 0)
template <class P> bool grow(eds_und* h, P*& p, size_t& have, size_t need) {
    if (have >= need) return true;
    if (p) { (void)hipStreamSynchronize(h->own.st); h->own.release(p); }
    have = 0;
    if (!h->own.alloc(p, need)) return false;
    have = need;
    return true;
}

int check_slot(const eds_und* h, int slot) {
    if (slot < 0 || slot >= h->slots) return fail(EDS_ERR_INVALID, "slot " + std::to_string(slot) + " of " + std::to_string(h->slots));
    return EDS_OK;
}

template <class T> void launch(eds_und* h, int form, const Frames& a, int count, float* out) {
    const edsund::Geometry& g = h->s.g;
    constexpr bool lds = sizeof(T) == 1;
    if (h->passthrough) {
        hipLaunchKernelGGL((k_und_plane<T, lds>), grid_of(g.w_org, g.h_org, count), dim3(TX, TY), 0, h->own.st, a, out);
    } else if (form == EDS_UND_FORM_FUSED) {
        hipLaunchKernelGGL((k_und_fused<T, lds>), grid_of(g.w, g.h, count), dim3(TX, TY), 0, h->own.st, a, h->d_map, out);
    } else {
        hipLaunchKernelGGL((k_und_plane<T, lds>), grid_of(g.w_org, g.h_org, count), dim3(TX, TY), 0, h->own.st, a, h->d_phot);
        hipLaunchKernelGGL(k_und_remap, grid_of(g.w, g.h, count), dim3(TX, TY), 0, h->own.st, h->d_phot, h->d_map, out, g.w_org, g.h_org, g.w, g.h);
    }
}

}  // namespace

extern "C" {

int eds_und_abi_version(void) { return EDS_HIP_UNDISTORT_ABI_VERSION; }

void eds_und_settings_default(eds_und_settings* s) {
    if (!s) return;
    const edsund::Settings d = edsund::settings_default();
    std::memcpy(s, &d, sizeof(d));
}

int eds_und_create(int device, const eds_und_geometry* geometry, int slots, eds_und** und) {
    if (!und) return fail(EDS_ERR_INVALID, "null output");
    *und = nullptr;
    if (!geometry) return fail(EDS_ERR_INVALID, "null geometry");
    if (slots < 1 || slots > edsund::MAX_SLOTS) return fail(EDS_ERR_INVALID, "slots are 1 .. 16");
    edsund::Geometry g;
    std::memcpy(&g, geometry, sizeof(g));
    if (!edsund::geometry_valid(g))
        return fail(EDS_ERR_INVALID, g.out_mode == edsund::OUT_FULL
                                         ? "output mode \"full\" does not exist (the reference asserts)"
                                         : "geometry: a model and an output mode that exist, sizes 8 .. 8192, finite parameters, mode \"none\" with equal sizes");
    eds_und* h = new eds_und;
    const int rc = edsund::setup(g, h->s);
    if (rc != edsund::RC_OK) {
        delete h;
        return rc == edsund::RC_NOT_USABLE ? fail(EDS_ERR_NOT_USABLE, "makeOptimalK_crop: no camera matrix after 500 iterations")
                                           : fail(EDS_ERR_INVALID, "geometry");
    }
    if (int rc2 = h->own.open(device)) { delete h; return rc2; }
    h->slots = slots;
    h->passthrough = h->s.passthrough;
    const size_t px = (size_t)g.w * g.h, px_org = (size_t)g.w_org * g.h_org;
    bool ok = h->own.alloc({{(void**)&h->d_map, px * sizeof(float2)},
                            {(void**)&h->d_planes, (size_t)slots * px * sizeof(float)},
                            {(void**)&h->d_G, (size_t)edsund::MAX_G_DEPTH * sizeof(float)},
                            {(void**)&h->d_vinv, px_org * sizeof(float)}}) &&
              hipMemsetAsync(h->d_planes, 0, (size_t)slots * px * sizeof(float), h->own.st) == hipSuccess &&
              hipMemsetAsync(h->d_G, 0, (size_t)edsund::MAX_G_DEPTH * sizeof(float), h->own.st) == hipSuccess &&
              hipMemsetAsync(h->d_vinv, 0, px_org * sizeof(float), h->own.st) == hipSuccess;
    ok = ok && upload_map(h, h->s.mapx.data(), h->s.mapy.data()) == EDS_OK;
    if (!ok) {
        (void)hipGetLastError();
        eds_und_destroy(h);
        return fail(EDS_ERR_HIP, "eds_und_create: the device refused a stream, an allocation or an upload");
    }
    *und = h;
    return EDS_OK;
}

void eds_und_destroy(eds_und* h) {
    if (!h) return;
    h->own.close();
    delete h;
}

int eds_und_get_K(const eds_und* h, double K[9]) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (!K) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(K, h->s.K, 9 * sizeof(double));
    return EDS_OK;
}

int eds_und_get_map(const eds_und* h, float* mapx, float* mapy) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    const size_t n = h->s.mapx.size() * sizeof(float);
    if (mapx) std::memcpy(mapx, h->s.mapx.data(), n);
    if (mapy) std::memcpy(mapy, h->s.mapy.data(), n);
    return EDS_OK;
}

int eds_und_is_passthrough(const eds_und* h, int* passthrough) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (!passthrough) return fail(EDS_ERR_INVALID, "null output");
    *passthrough = h->passthrough ? 1 : 0;
    return EDS_OK;
}

int eds_und_set_map(eds_und* h, const float* mapx, const float* mapy) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (!mapx || !mapy) return fail(EDS_ERR_INVALID, "map: NULL pointer");
    const edsund::Geometry& g = h->s.g;
    const size_t n = (size_t)g.w * g.h;
    if (!edsund::map_valid(mapx, mapy, n, g.w_org, g.h_org))
        return fail(EDS_ERR_INVALID, "map: every pair is (-1, -1) or finite with 0 < x < w_org - 1 and 0 < y < h_org - 1");
    if (int rc = upload_map(h, mapx, mapy)) return rc;
    h->s.mapx.assign(mapx, mapx + n);
    h->s.mapy.assign(mapy, mapy + n);
    h->passthrough = false;
    return EDS_OK;
}

int eds_und_set_photometric(eds_und* h, const float* G, int g_depth, const void* vignette, int vignette_type) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    const size_t n = (size_t)h->s.g.w_org * h->s.g.h_org;
    edsund::Photometric p;
    if (edsund::set_photometric(p, G, g_depth, vignette, vignette_type, n, h->st.photometric_calibration) != edsund::RC_OK)
        return fail(EDS_ERR_INVALID, "photometric calibration: G of 256 .. 65536 strictly increasing floats, a vignette of uint8 or uint16");
    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_vinv, p.vignetteMapInv.data(), n * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipMemcpyAsync(h->d_G, p.G.data(), (size_t)p.g_depth * sizeof(float), hipMemcpyHostToDevice, h->own.st));
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    h->ph = std::move(p);
    return EDS_OK;
}

int eds_und_set_settings(eds_und* h, const eds_und_settings* s) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (!s) return fail(EDS_ERR_INVALID, "null settings");
    edsund::Settings v;
    std::memcpy(&v, s, sizeof(v));
    if (!edsund::settings_valid(v)) return fail(EDS_ERR_INVALID, "settings: photometric_calibration 0 .. 2, use_exposure 0 or 1");
    const bool table_changes = h->ph.valid && (v.photometric_calibration == 0) != (h->st.photometric_calibration == 0);
    h->st = v;
    if (table_changes) {
        edsund::apply_mode_to_G(h->ph, v.photometric_calibration);
        if (int rc = upload_G(h)) return rc;
    }
    return EDS_OK;
}

int eds_und_get_settings(const eds_und* h, eds_und_settings* s) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (!s) return fail(EDS_ERR_INVALID, "null output");
    std::memcpy(s, &h->st, sizeof(*s));
    return EDS_OK;
}

int eds_und_set_form(eds_und* h, int form) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (form != EDS_UND_FORM_FUSED && form != EDS_UND_FORM_TWO_PASS && form != EDS_UND_FORM_AUTO)
        return fail(EDS_ERR_INVALID, "form is EDS_UND_FORM_FUSED, EDS_UND_FORM_TWO_PASS or EDS_UND_FORM_AUTO");
    h->form = form;
    return EDS_OK;
}

int eds_und_get_form(const eds_und* h, int* form) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (!form) return fail(EDS_ERR_INVALID, "null output");
    *form = h->form;
    return EDS_OK;
}

int eds_und_process(eds_und* h, int first_slot, int count, const void* raw, int raw_type, int64_t rs, int64_t fs, int on_device,
                    const float* exposures, float factor, float* exposures_out) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    const edsund::Geometry& g = h->s.g;
    if (count < 1 || first_slot < 0 || first_slot > h->slots - count)
        return fail(EDS_ERR_INVALID, "slots " + std::to_string(first_slot) + " .. +" + std::to_string(count) + " of " + std::to_string(h->slots));
    if (!raw) return fail(EDS_ERR_INVALID, "raw: NULL pointer");
    if (!exposures) return fail(EDS_ERR_INVALID, "exposures: NULL pointer");
    if (raw_type != EDS_UND_U8 && raw_type != EDS_UND_U16) return fail(EDS_ERR_INVALID, "raw_type is EDS_UND_U8 or EDS_UND_U16");
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    const size_t elem = raw_type == EDS_UND_U16 ? 2 : 1;
    if (rs == 0) rs = g.w_org;
    if (rs < g.w_org || rs > (int64_t)1 << 30) return fail(EDS_ERR_INVALID, "bad row stride");
    const int64_t extent = (int64_t)(g.h_org - 1) * rs + g.w_org;
    if (fs == 0) fs = (int64_t)g.h_org * rs;
    if (fs < extent || fs > (int64_t)1 << 40) return fail(EDS_ERR_INVALID, "bad frame stride");
    if (reinterpret_cast<uintptr_t>(raw) % elem) return fail(EDS_ERR_INVALID, "raw: uint16 frames not aligned to 2 bytes");
    if (!edsund::raw_type_fits(h->ph, h->st.photometric_calibration, raw_type))
        return fail(EDS_ERR_INVALID, "uint16 frames with the photometric calibration on need a G table of 65536 entries, not " + std::to_string(h->ph.g_depth));
    const size_t bytes = (size_t)((int64_t)(count - 1) * fs + extent) * elem;
    if (on_device)
        if (int rc = eds_dev_check_range(h->own.dev, raw, bytes)) return rc;

    EDS_HIP_TRY(hipSetDevice(h->own.dev));
    const size_t px_org = (size_t)g.w_org * g.h_org;
    if (!on_device && !grow(h, h->d_raw, h->raw_bytes, (size_t)count * px_org * elem))
        return fail(EDS_ERR_HIP, "eds_und_process: the device refused the staging buffer");
    const int form = h->form != EDS_UND_FORM_AUTO ? h->form : (int64_t)count * (int64_t)px_org >= AUTO_TWO_PASS_PIXELS ? EDS_UND_FORM_TWO_PASS : EDS_UND_FORM_FUSED;
    if (!h->passthrough && form == EDS_UND_FORM_TWO_PASS && !grow(h, h->d_phot, h->phot_bytes, (size_t)count * px_org * sizeof(float)))
        return fail(EDS_ERR_HIP, "eds_und_process: the device refused the photometric planes");

    Frames a;
    a.raw = raw; a.rs = rs; a.fs = fs;
    if (!on_device) {
        for (int k = 0; k < count; ++k)
            EDS_HIP_TRY(hipMemcpy2DAsync(static_cast<char*>(h->d_raw) + (size_t)k * px_org * elem, (size_t)g.w_org * elem,
                                         static_cast<const char*>(raw) + (size_t)k * fs * elem, (size_t)rs * elem, (size_t)g.w_org * elem,
                                         (size_t)g.h_org, hipMemcpyHostToDevice, h->own.st));
        a.raw = h->d_raw; a.rs = g.w_org; a.fs = (int64_t)px_org;
    }
    a.phot_mask = 0;
    for (int k = 0; k < count; ++k)
        if (edsund::photometric_branch(h->ph.valid, exposures[k], h->st.photometric_calibration)) a.phot_mask |= 1u << k;
    a.vig = h->st.photometric_calibration == 2;
    a.factor = factor;
    a.G = h->d_G; a.vinv = h->d_vinv;
    a.w_org = g.w_org; a.h_org = g.h_org; a.w = g.w; a.h = g.h;
    float* out = h->d_planes + (size_t)first_slot * g.w * g.h;
    if (raw_type == EDS_UND_U16) launch<uint16_t>(h, form, a, count, out);
    else launch<uint8_t>(h, form, a, count, out);
    EDS_HIP_TRY(hipGetLastError());
    EDS_HIP_TRY(hipStreamSynchronize(h->own.st));
    if (exposures_out)
        for (int k = 0; k < count; ++k) exposures_out[k] = h->st.use_exposure ? exposures[k] : 1.0f;
    return EDS_OK;
}

int eds_und_image(const eds_und* h, int slot, const float** d_image, int64_t* row_stride) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (int rc = check_slot(h, slot)) return rc;
    if (!d_image) return fail(EDS_ERR_INVALID, "null output");
    *d_image = h->d_planes + (size_t)slot * h->s.g.w * h->s.g.h;
    if (row_stride) *row_stride = h->s.g.w;
    return EDS_OK;
}

int eds_und_get_image(eds_und* h, int slot, float* out) {
    if (int rc = edscapi::check_handle(h, "eds_und")) return rc;
    if (int rc = check_slot(h, slot)) return rc;
    if (!out) return fail(EDS_ERR_INVALID, "null output");
    const size_t px = (size_t)h->s.g.w * h->s.g.h;
    return read_back(h->own, out, h->d_planes + (size_t)slot * px, px * sizeof(float));
}

}  // extern "C"
