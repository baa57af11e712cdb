// csrc/eds_inisetup.hpp (namespace edsini: gridMaxSelection and makePixelStatus as the host restates them) behind a C interface for ctypes.
// Loaded through tests/inisetup_harness.py; -DINISETUP_STANDALONE makes a program with its own main and its own inputs (the sanitizer run).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../slam-eds_amd/csrc/eds_inisetup.hpp"

using namespace edsini;

namespace {
// h x w x {colour, dx, dy} floats as the Px records the library holds
std::vector<Px> to_px(const float* g, int w, int h) {
    std::vector<Px> p((size_t)w * h);
    for (size_t i = 0; i < p.size(); ++i) { p[i].c = g[3 * i]; p[i].dx = g[3 * i + 1]; p[i].dy = g[3 * i + 2]; p[i].pad = 0.0f; }
    return p;
}
}  // namespace

extern "C" {

int inisetup_cells(int w, int pot) { return gms_cells(w, pot); }

int inisetup_grid_max_selection(const float* grads, int w, int h, int pot, float th_fac, uint8_t* map) {
    const std::vector<Px> p = to_px(grads, w, h);
    return grid_max_selection(p.data(), map, w, h, pot, th_fac);
}

int inisetup_make_pixel_status(const float* grads, int w, int h, float desired, int recs_left, float th_fac, int32_t* sparsity, int32_t* passes,
                               uint8_t* map) {
    const std::vector<Px> p = to_px(grads, w, h);
    return make_pixel_status(p.data(), map, w, h, desired, recs_left, th_fac, sparsity, passes);
}

}  // extern "C"

#ifdef INISETUP_STANDALONE
int main() {
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    long total = 0, calls = 0;
    const int shapes[4][2] = {{48, 40}, {9, 8}, {8, 8}, {33, 17}};
    for (int k = 0; k < 4; ++k) {
        const int w = shapes[k][0], h = shapes[k][1];
        std::vector<float> g((size_t)w * h * 3);
        for (size_t i = 0; i < g.size(); ++i) g[i] = 60.0f * rnd() - 30.0f;
        g[4] = NAN; g[8] = INFINITY; g[10] = -INFINITY; g[11] = INFINITY;       // hostile gradients: never selected, never read out of bounds
        std::vector<uint8_t> map((size_t)w * h);
        for (int pot : {1, 2, 3, 7, 8, 9, 11, 13, h - 2, h - 1, h, 1000, 1 << 30}) {
            total += inisetup_grid_max_selection(g.data(), w, h, pot, 1.0f, map.data());
            ++calls;
        }
        for (float desired : {1e-30f, 1.0f, 50.0f, 1e9f})
            for (int32_t start : {-3, 1, 5, 1 << 30}) {
                int32_t sp = start, passes = 0;
                total += inisetup_make_pixel_status(g.data(), w, h, desired, 5, 1.0f, &sp, &passes, map.data());
                if (sp < 1 || passes < 1 || passes > 6) return 1;
                ++calls;
            }
    }
    printf("inisetup standalone: %ld calls, %ld points\n", calls, total);
    return 0;
}
#endif
