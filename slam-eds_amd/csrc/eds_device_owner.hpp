// What the host code of the DSO-side handles shares (eds_imm, eds_ct, eds_win, eds_sel and the eds_act / eds_wsv / eds_wed states that hang
// off them): one owner for a handle's device, stream and device memory, the check and upload of caller images, the read-back, and the
// small argument checks.  Host code only; the one kernel pair the handles share, a level of makeImages, is eds_dso_image.hip's and is
// queued through queue_level below.  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>

#include "../../include/eds_hip.h"
#include "../../include/eds_hip_device.h"

namespace edsdso { struct Px; }

namespace edscapi {

int fail(int code, const std::string& msg);          // records the message for eds_last_error() (thread-local), returns `code`

#define EDS_HIP_TRY(expr)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return edscapi::fail(EDS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

struct DevAlloc { void** p; size_t bytes; };

#pragma GCC visibility push(hidden)                   // inline host code: none of it joins the library's exported symbols

// The device, the stream and every hipMalloc of one handle.  It records pointer VALUES, not the addresses of the fields that hold them,
// so fields may exchange their pointers (eds_winedit.hip) and close() still frees each buffer once.  Plain data: a handle holds one by
// value and calls close() itself.
struct DeviceOwner {
    int dev = 0;
    hipStream_t st = nullptr;
    void** owned = nullptr;
    size_t n_owned = 0, cap = 0;

    // EDS_ERR_NO_DEVICE, EDS_ERR_INVALID for the ordinal, EDS_ERR_HIP when the device cannot be selected.  A refused stream is not an
    // error here: st stays NULL, every alloc() then returns false, and the creator reports "refused a stream or an allocation" once.
    int open(int device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
            (void)hipGetLastError();
            return fail(EDS_ERR_NO_DEVICE, "no HIP device");
        }
        if (device < 0 || device >= ndev) return fail(EDS_ERR_INVALID, "device " + std::to_string(device) + " of " + std::to_string(ndev));
        EDS_HIP_TRY(hipSetDevice(device));
        dev = device;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st = nullptr; }
        return EDS_OK;
    }

    size_t live() const { return n_owned; }

    // hipMalloc, recorded; false (p untouched, the runtime's error cleared) when the device or the owner refuses
    template <class T> bool alloc(T*& p, size_t bytes) {
        if (!st) return false;
        if (n_owned == cap) {
            void** grown = static_cast<void**>(std::realloc(owned, (cap + 32) * sizeof(void*)));
            if (!grown) return false;
            owned = grown; cap += 32;
        }
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess || !q) { (void)hipGetLastError(); return false; }
        owned[n_owned++] = q;
        p = static_cast<T*>(q);
        return true;
    }
    // every entry in turn; at the first that fails the entries before it are freed again, every entry is NULL, and the answer is false
    bool alloc(std::initializer_list<DevAlloc> table) {
        const size_t mark = n_owned;
        for (const DevAlloc& a : table)
            if (!alloc(*a.p, a.bytes)) {
                release_from(mark);
                for (const DevAlloc& b : table) *b.p = nullptr;
                return false;
            }
        return true;
    }

    // frees one recorded pointer; p is NULL afterwards (a pointer that was never recorded is only set to NULL)
    template <class T> void release(T*& p) {
        for (size_t i = 0; i < n_owned; ++i)
            if (owned[i] == p) {
                (void)hipFree(owned[i]);
                std::memmove(owned + i, owned + i + 1, (--n_owned - i) * sizeof(void*));
                break;
            }
        p = nullptr;
    }
    // frees what was recorded since live() was `mark`: a state that did not come to life
    void release_from(size_t mark) {
        while (n_owned > mark) (void)hipFree(owned[--n_owned]);
    }

    // waits for the stream, frees everything recorded, destroys the stream.  Harmless on an owner that never opened, and twice.
    void close() {
        if (st) {
            (void)hipSetDevice(dev);
            (void)hipStreamSynchronize(st);
            release_from(0);
            (void)hipStreamDestroy(st);
        }
        std::free(owned);
        owned = nullptr; st = nullptr; n_owned = cap = 0;
    }
};

inline int check_handle(const void* h, const char* type) { return h ? EDS_OK : fail(EDS_ERR_INVALID, std::string("null ") + type + " handle"); }

inline unsigned blocks(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// fx, fy, cx, cy finite, fx and fy > 0
inline bool check_calib(float fx, float fy, float cx, float cy) {
    return std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy) && fx > 0.0f && fy > 0.0f;
}

// What a call checks of `count` caller images of H x W floats before anything changes, short of the device range: the pointer, on_device
// 0 or 1, the strides in floats (0: dense; *rs and *fs become the effective ones), 4-byte alignment.  fs == NULL: one image, no frame
// stride.  `what` is the argument's name in the messages; `strides`, when given, is the one message for either stride.  *bytes: the
// extent a device pointer is then checked over.
inline int check_image_layout(int H, int W, int count, const float* images, int64_t* rs, int64_t* fs, int on_device, const char* what,
                              const char* strides, size_t* bytes) {
    if (!images) return fail(EDS_ERR_INVALID, std::string(what) + ": NULL pointer");
    if (on_device != 0 && on_device != 1) return fail(EDS_ERR_INVALID, "on_device is 0 or 1");
    if (*rs == 0) *rs = W;
    const bool rs_bad = *rs < W || *rs > (int64_t)1 << 30;
    if (rs_bad && !strides) return fail(EDS_ERR_INVALID, "bad row stride");
    const int64_t extent = (int64_t)(H - 1) * *rs + W;
    int64_t frames = 0;
    if (fs) {
        if (*fs == 0) *fs = (int64_t)H * *rs;
        if (rs_bad || *fs < extent || *fs > (int64_t)1 << 40) return fail(EDS_ERR_INVALID, strides ? strides : "bad frame stride");
        frames = (int64_t)(count - 1) * *fs;
    }
    if (reinterpret_cast<uintptr_t>(images) % sizeof(float)) return fail(EDS_ERR_INVALID, std::string(what) + ": not aligned to 4 bytes");
    *bytes = (size_t)(frames + extent) * sizeof(float);
    return EDS_OK;
}
// ... and with the range: eds_dev_check_range over the whole extent when the images are in device memory
inline int check_images(int dev, int H, int W, int count, const float* images, int64_t* rs, int64_t* fs, int on_device, const char* what,
                        const char* strides = nullptr) {
    size_t bytes = 0;
    if (int rc = check_image_layout(H, W, count, images, rs, fs, on_device, what, strides, &bytes)) return rc;
    return on_device ? eds_dev_check_range(dev, images, bytes) : (int)EDS_OK;
}
// one checked image into the dense H x W plane `dst`, queued into the owner's stream
inline int upload_image(const DeviceOwner& o, float* dst, int H, int W, const float* src, int64_t rs, int on_device) {
    EDS_HIP_TRY(hipMemcpy2DAsync(dst, (size_t)W * sizeof(float), src, (size_t)rs * sizeof(float), (size_t)W * sizeof(float), (size_t)H,
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, o.st));
    return EDS_OK;
}

// eds_dso_image.hip: one level of makeImages (w x h, at `out`) queued into st, nothing waited for: its colours from the dense image `img`
// (level 0, lm NULL) or from the level below (lm, wlm1 wide), then its gradients.  Two launches of blocks(w * h) workgroups;
// queue_colours is the first alone, for eds_sel, whose own gradient kernel also writes absSquaredGrad.
void queue_colours(hipStream_t st, const float* img, const edsdso::Px* lm, int wlm1, edsdso::Px* out, int w, int h);
void queue_level(hipStream_t st, const float* img, const edsdso::Px* lm, int wlm1, edsdso::Px* out, int w, int h);

// device memory into the caller's, waited for; a NULL dst or no bytes is no work
inline int read_back(const DeviceOwner& o, void* dst, const void* src, size_t bytes) {
    if (!dst || !bytes) return EDS_OK;
    EDS_HIP_TRY(hipSetDevice(o.dev));
    EDS_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, o.st));
    EDS_HIP_TRY(hipStreamSynchronize(o.st));
    return EDS_OK;
}

#pragma GCC visibility pop

}  // namespace edscapi
