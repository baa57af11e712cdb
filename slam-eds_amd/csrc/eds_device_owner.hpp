// What the host code of the handles shares (eds_trk and the Eds*Buffers structs that hang off it; eds_imm, eds_ct, eds_win, eds_sel, eds_ini,
// eds_und and the eds_act / eds_wsv / eds_wed states beside them): one owner for a handle's device, stream, device memory and pinned host
// memory, the check and upload of caller images, the read-back, and the small argument checks.  Host code only; the one kernel pair the
// DSO-side handles share, a level of makeImages, is eds_dso_image.hip's and is queued through queue_level below.  Nothing here is part of
// the ABI.
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

// One entry of an alloc() / regrow() table: hipMalloc when `host` is DEVICE; pinned host memory otherwise, and for MAPPED *view receives the
// device's pointer to the same block.  pinned() and mapped() spell the latter two.
struct DevAlloc {
    enum Kind { DEVICE, PINNED, MAPPED };
    void** p; size_t bytes; Kind host = DEVICE; void** view = nullptr;
};

#pragma GCC visibility push(hidden)                   // inline host code: none of it joins the library's exported symbols

template <class T> DevAlloc pinned(T*& p, size_t bytes) { return {(void**)&p, bytes, DevAlloc::PINNED, nullptr}; }
template <class T, class U> DevAlloc mapped(T*& host, U*& dev, size_t bytes) { return {(void**)&host, bytes, DevAlloc::MAPPED, (void**)&dev}; }

// The device, the stream and every hipMalloc and hipHostMalloc of one handle, in two lists.  It records pointer VALUES, not the addresses
// of the fields that hold them, so fields may exchange their pointers (eds_winedit.hip) and close() still frees each buffer once.  Plain
// data: a handle holds one by value and calls close() itself.
struct DeviceOwner {
    int dev = 0;
    hipStream_t st = nullptr;
    struct List { void** v = nullptr; size_t n = 0, cap = 0; };
    List owned, pins;                                 // device memory; pinned host memory

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

    size_t live() const { return owned.n; }
    size_t live_pinned() const { return pins.n; }

    // room for one more entry; false when the owner never opened or the host refuses
    bool room(List& l) {
        if (!st) return false;
        if (l.n == l.cap) {
            void** grown = static_cast<void**>(std::realloc(l.v, (l.cap + 32) * sizeof(void*)));
            if (!grown) return false;
            l.v = grown; l.cap += 32;
        }
        return true;
    }
    // hipMalloc, recorded; false (p untouched, the runtime's error cleared) when the device or the owner refuses
    template <class T> bool alloc(T*& p, size_t bytes) {
        void* q = nullptr;
        if (!room(owned)) return false;
        if (hipMalloc(&q, bytes) != hipSuccess || !q) { (void)hipGetLastError(); return false; }
        owned.v[owned.n++] = q;
        p = static_cast<T*>(q);
        return true;
    }
    // hipHostMalloc, recorded in the second list; refusal as above
    template <class T> bool alloc_pinned(T*& host, size_t bytes, unsigned flags = hipHostMallocDefault) {
        void* q = nullptr;
        if (!room(pins)) return false;
        if (hipHostMalloc(&q, bytes, flags) != hipSuccess || !q) { (void)hipGetLastError(); return false; }
        pins.v[pins.n++] = q;
        host = static_cast<T*>(q);
        return true;
    }
    // the device's pointer to a pinned block, NULL (the runtime's error cleared) when it has none
    template <class T> T* device_view(T* host) {
        void* d = nullptr;
        if (!host || hipHostGetDevicePointer(&d, host, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return static_cast<T*>(d);
    }
    // pinned and device-mapped: the block and the device's pointer to it, or neither (the block freed again, both NULL, the error cleared)
    template <class T, class U> bool alloc_mapped(T*& host, U*& dev_view, size_t bytes) {
        void* q = nullptr;
        host = nullptr; dev_view = nullptr;
        if (!alloc_pinned(q, bytes, hipHostMallocMapped)) return false;
        void* d = device_view(q);
        if (!d) { release(q); return false; }
        host = static_cast<T*>(q); dev_view = static_cast<U*>(d);
        return true;
    }
    // every entry in turn; at the first that fails the entries before it are freed again, every entry is NULL, and the answer is false
    bool alloc(std::initializer_list<DevAlloc> table) {
        const size_t mark = owned.n, pin_mark = pins.n;
        for (const DevAlloc& a : table)
            if (!(a.host == DevAlloc::DEVICE ? alloc(*a.p, a.bytes) : a.host == DevAlloc::PINNED ? alloc_pinned(*a.p, a.bytes) : alloc_mapped(*a.p, *a.view, a.bytes))) {
                release_from(mark, pin_mark);
                for (const DevAlloc& b : table) { *b.p = nullptr; if (b.view) *b.view = nullptr; }
                return false;
            }
        return true;
    }
    // Grows what a capacity field counts: releases the table's buffers, then allocates them at the sizes the caller worked out for `want`.
    // On refusal every entry is NULL and cap is 0, so the caller's next "cap >= need" test cannot believe in a buffer that is gone.
    template <class Cap> bool regrow(Cap& cap, Cap want, std::initializer_list<DevAlloc> table) {
        for (const DevAlloc& a : table) { release(*a.p); if (a.view) *a.view = nullptr; }
        cap = alloc(table) ? want : Cap(0);
        return cap != Cap(0);
    }

    // frees one recorded pointer of either list; p is NULL afterwards (a pointer that was never recorded is only set to NULL)
    template <class T> void release(T*& p) {
        if (p && !drop(owned, p, false)) drop(pins, p, true);
        p = nullptr;
    }
    bool drop(List& l, const void* p, bool host) {
        for (size_t i = 0; i < l.n; ++i)
            if (l.v[i] == p) {
                (void)(host ? hipHostFree(l.v[i]) : hipFree(l.v[i]));
                std::memmove(l.v + i, l.v + i + 1, (--l.n - i) * sizeof(void*));
                return true;
            }
        return false;
    }
    // frees what was recorded since live() was `mark` (and live_pinned() `pin_mark`, when given): a state that did not come to life
    void release_from(size_t mark, size_t pin_mark = SIZE_MAX) {
        while (owned.n > mark) (void)hipFree(owned.v[--owned.n]);
        while (pins.n > pin_mark) (void)hipHostFree(pins.v[--pins.n]);
    }

    // waits for the stream, frees everything recorded, destroys the stream.  Harmless on an owner that never opened, and twice.
    void close() {
        if (st) {
            (void)hipSetDevice(dev);
            (void)hipStreamSynchronize(st);
            release_from(0, 0);
            (void)hipStreamDestroy(st);
        }
        std::free(owned.v); std::free(pins.v);
        owned = pins = List();
        st = nullptr;
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
