// slam-eds_amd/csrc/eds_dso_common.hpp under g++, for tests/test_dso_common.py: a frame's levels and the interpolation of {c, dx, dy}
#include "../../slam-eds_amd/csrc/eds_dso_common.hpp"

using edsdso::Px;

extern "C" {

// out: the levels one after the other, (w >> l) * (h >> l) pixels of four floats each
void dso_make_levels(const float* image, int64_t row_stride, int w, int h, int levels, float* out) {
    Px* lv[8];
    Px* p = reinterpret_cast<Px*>(out);
    for (int l = 0; l < levels && l < 8; ++l) { lv[l] = p; p += (size_t)(w >> l) * (h >> l); }
    edsdso::make_levels(image, row_stride, w, h, levels < 8 ? levels : 8, lv);
}

// getInterpolatedElement33 of n samples xy[2 i], xy[2 i + 1] inside a level w wide: out[3 i ..] = colour, dx, dy
void dso_interp33(const float* level, int w, int n, const float* xy, float* out) {
    const Px* px = reinterpret_cast<const Px*>(level);
    for (int i = 0; i < n; ++i) {
        const edsdso::Bilin b = edsdso::bilin(xy[2 * i], xy[2 * i + 1]);
        const Px* bp = px + ((size_t)b.iy * w + b.ix);
        out[3 * i] = edsdso::mix(b, bp[1 + w].c, bp[w].c, bp[1].c, bp[0].c);
        out[3 * i + 1] = edsdso::mix(b, bp[1 + w].dx, bp[w].dx, bp[1].dx, bp[0].dx);
        out[3 * i + 2] = edsdso::mix(b, bp[1 + w].dy, bp[w].dy, bp[1].dy, bp[0].dy);
    }
}

}
