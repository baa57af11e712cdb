// One level of makeImages on the device, for every DSO-side handle that keeps frames as Px (eds_ct, eds_win, eds_sel): the level's
// colours, then its gradients.  The arithmetic is eds_dso_common.hpp's, shared with the host.  Built without contraction into FMAs
// (csrc/Makefile).
#include <hip/hip_runtime.h>

#include "eds_device_owner.hpp"
#include "eds_dso_common.hpp"

using edsdso::Px;

namespace {

constexpr int TB = 256;

__global__ void __launch_bounds__(TB) k_px_level(const float* __restrict__ img, const Px* __restrict__ lm, int wlm1, Px* __restrict__ out, int w,
                                                 int n) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    out[i] = edsdso::level_pixel(img, lm, wlm1, w, i);
}

__global__ void __launch_bounds__(TB) k_px_gradient(Px* px, int w, int h) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= w * h) return;
    float dx, dy;
    edsdso::gradient_at(px, w, h, i, &dx, &dy);
    px[i].dx = dx;
    px[i].dy = dy;
}

}  // namespace

namespace edscapi {

void queue_colours(hipStream_t st, const float* img, const Px* lm, int wlm1, Px* out, int w, int h) {
    hipLaunchKernelGGL(k_px_level, dim3(blocks((int64_t)w * h)), dim3(TB), 0, st, img, lm, wlm1, out, w, w * h);
}

void queue_level(hipStream_t st, const float* img, const Px* lm, int wlm1, Px* out, int w, int h) {
    queue_colours(st, img, lm, wlm1, out, w, h);
    hipLaunchKernelGGL(k_px_gradient, dim3(blocks((int64_t)w * h)), dim3(TB), 0, st, out, w, h);
}

}  // namespace edscapi
